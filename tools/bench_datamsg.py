"""Whole NORM_DATA messages on the device against the payload-and-ID calls and the streaming copy.

Five candidates work on the same transmission list, laid out with 32 bytes in front of every payload
(the header of fec_id 5 with its FTI extension, the reference's default sender):
  (a) nfec_tx_emit_data: the 32-byte header and the payload of every listed slot;
  (b) nfec_tx_emit with the same list: the 4-byte payload ID and the payload (28 bytes per message
      left to the host);
  (c) nfec_rx_ingest_data on (a)'s wire buffer and datagram table, in shuffled arrival order;
  (d) nfec_rx_ingest on (b)'s wire buffer, the same payload bytes laid out its way (ID in front of
      the payload, payload offsets known), in the same order;
  (e) nfec_util_stream_copy of the bytes (a) writes and (c) reads.
They alternate in `--rounds` rounds; every candidate of a round is timed with HIP events around each
of `--iters` calls (the mean is the round's figure) after `--warmup` untimed calls.  The reception
masks are re-zeroed ahead of every call of (c) and (d), outside the timed region.

This is a report, not a gate: the line records each new call's time over its parent call's per round,
the parent calls' own round-to-round spread, and whether the new call stays within that spread plus
5 %.  Only a comparison inside one run counts.

Shape: RS8(64, 32), 1,400-byte vectors, 65,536 blocks, 80 of 96 segments of every block.

One JSON line is appended to --out (default profiles/datamsg/datamsg.jsonl) and printed.  A run
without a GPU fails.

  python3 tools/bench_datamsg.py
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--blocks", type=int, default=65536)
    p.add_argument("--k", type=int, default=64)
    p.add_argument("--m", type=int, default=32)
    p.add_argument("--vec", type=int, default=1400)
    p.add_argument("--sent", type=int, default=80, help="segments of every block that are sent and arrive")
    p.add_argument("--first-block-id", type=lambda s: int(s, 0), default=0xFFF000,
                   help="the window wraps fec_id 5's 24-bit block field inside the batch")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "datamsg", "datamsg.jsonl"))
    a = p.parse_args()

    import numpy as np
    import torch
    import norm_amd as na
    from norm_amd import wire as W

    if not torch.cuda.is_available() or na.device_count() < 1:
        raise SystemExit("bench_datamsg: needs an MI355X")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    k, m, nb, vec = a.k, a.m, a.blocks, a.vec
    fec_id, fec_m = 5, 8
    enc = na.NormEncoderRS8()
    assert enc.Init(k, m, vec)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0x4E4F524D)

    fti = W.write_fti(W.FecObjectInfo(fec_id, vec - 8, k, m, object_size=nb * k * (vec - 8), fec_m=fec_m))
    H = na.data_header_bytes(fec_id, len(fti))
    header = na.data_header(0xC0A80107, 0x1234, 7, fec_id, fec_m, first_sequence=65000, grtt=0x9C, backoff=4, gsize=3,
                            flags=0x18, fti=fti)
    flt = na.data_filter(0xC0A80107, 0x1234, 7, fec_id, fec_m)

    # the sender's batch (any bytes: nothing here encodes or decodes) and its pending mask
    sent = torch.empty((nb, k + m, vec), dtype=torch.uint8, device="cuda")
    flat = sent.view(-1)
    for at in range(0, flat.numel(), 1 << 28):
        part = flat[at:at + (1 << 28)]
        part.copy_(torch.randint(0, 256, (part.numel(),), dtype=torch.uint8, device="cuda", generator=gen))
    words = (k + m + 31) // 32
    rank = torch.rand((nb, k + m), device="cuda", generator=gen).argsort(dim=1).argsort(dim=1)
    bits = torch.zeros((nb, words * 32), dtype=torch.int64, device="cuda")
    bits[:, :k + m] = (rank < a.sent).to(torch.int64)
    word = (bits.view(nb, words, 32) << torch.arange(32, device="cuda")).sum(dim=2)
    pending = torch.where(word >= 1 << 31, word - (1 << 32), word).to(torch.int32).contiguous()
    del rank, bits, word
    count = nb * a.sent
    nbytes = count * (H + vec)
    off, blk, sym, ln, start = enc.list_pending(pending, gap=H, capacity=count)
    torch.cuda.synchronize()
    assert start[nb].tolist() == [count, nbytes], start[nb].tolist()
    del pending

    wire_new = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")  # ends with its last message
    wire_old = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    m_off = torch.zeros(count, dtype=torch.int64, device="cuda")
    m_len = torch.zeros(count, dtype=torch.int16, device="cuda")
    tstats = torch.zeros(2, dtype=torch.int32, device="cuda")

    def emit_data():
        enc.emit_data_messages(sent, wire_new, off, blk, sym, ln, header, count_dev=start[nb, :1],
                               first_block_id=a.first_block_id, msg_offsets_out=m_off, msg_length_out=m_len, stream=stream)

    def emit():
        enc.emit_segments(sent, wire_old, off, blk, sym, ln, count_dev=start[nb, :1], fec_id=fec_id, fec_m=fec_m,
                          first_block_id=a.first_block_id, stream=stream)

    enc.emit_data_messages(sent, wire_new, off, blk, sym, ln, header, count_dev=start[nb, :1],
                           first_block_id=a.first_block_id, msg_offsets_out=m_off, msg_length_out=m_len, stats=tstats,
                           stream=stream)
    emit()
    torch.cuda.synchronize()
    emitted_ok = tstats.tolist() == [count, 0]
    # the payloads and their IDs are the same bytes in both buffers
    idx = torch.randint(0, count, (4096,), device="cuda", generator=gen)
    at = off[idx][:, None] + torch.arange(vec, device="cuda")[None, :]
    same_payloads = bool(torch.equal(wire_new[at], wire_old[at]))
    ids_new = wire_new[(off[idx] - H + 16)[:, None] + torch.arange(4, device="cuda")[None, :]]
    ids_old = wire_old[(off[idx] - 4)[:, None] + torch.arange(4, device="cuda")[None, :]]
    same_ids = bool(torch.equal(ids_new, ids_old))
    del idx, at, ids_new, ids_old

    # arrival order: shuffled over the whole batch
    order = torch.randperm(count, device="cuda", generator=gen)
    d_off, d_len = m_off[order].contiguous(), m_len[order].contiguous()
    p_off, p_len = off[order].contiguous(), ln[order].contiguous()
    want_blk, want_sym = blk[order], sym[order]
    del order

    batch_a = torch.empty_like(sent)
    batch_b = torch.empty_like(sent)
    batch_a.fill_(0x5A)
    batch_b.fill_(0x5A)
    mask_a, mask_b = na.received_mask(nb, k, m), na.received_mask(nb, k, m)
    block_index = torch.empty(count, dtype=torch.int32, device="cuda")
    symbol_id = torch.empty(count, dtype=torch.int16, device="cuda")
    rstats = torch.zeros(9, dtype=torch.int32, device="cuda")
    totals = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    enc.ingest_datagrams(batch_a, mask_a, wire_new, d_off, d_len, flt, first_block_id=a.first_block_id,
                         block_index_out=block_index, symbol_id_out=symbol_id, stats=rstats, totals=totals,
                         stream=stream)
    torch.cuda.synchronize()
    parsed_ok = bool(torch.equal(block_index, want_blk)) and bool(torch.equal(symbol_id, want_sym))
    placed_ok = rstats.tolist() == [0] * 8 + [count] and int(totals.item()) == 0
    del want_blk, want_sym, block_index, symbol_id

    def ingest_data():
        enc.ingest_datagrams(batch_a, mask_a, wire_new, d_off, d_len, flt, first_block_id=a.first_block_id, stream=stream)

    def ingest():
        enc.ingest_messages(batch_b, mask_b, wire_old, p_off, p_len, fec_id, fec_m, first_block_id=a.first_block_id,
                            stream=stream)

    copy_bytes = nbytes & ~15
    cdst = wire_old[:copy_bytes]
    csrc = wire_new[:copy_bytes]
    cands = [
        ("tx_emit_data", emit_data, None),
        ("tx_emit", emit, None),
        ("rx_ingest_data", ingest_data, lambda: mask_a.zero_()),
        ("rx_ingest", ingest, lambda: mask_b.zero_()),
    ]

    def timed(fn, before):
        for _ in range(a.warmup):
            if before:
                before()
            fn()
        total = 0.0
        for _ in range(a.iters):
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            total += e0.elapsed_time(e1)
        return total / a.iters

    rounds = [{name: timed(fn, before) for name, fn, before in cands} for _ in range(a.rounds)]
    same = all(bool(torch.equal(batch_a[b0:b0 + 4096], batch_b[b0:b0 + 4096])) for b0 in range(0, nb, 4096))
    same = same and bool(torch.equal(mask_a, mask_b))
    # the copy last: it overwrites the parent's wire buffer, which has served its purpose
    copy_ms = [timed(lambda: na.stream_copy(cdst, csrc, stream=stream), None) for _ in range(a.rounds)]
    for r, c in zip(rounds, copy_ms):
        r["stream_copy"] = c

    def spread(name):
        v = [r[name] for r in rounds]
        return (max(v) - min(v)) / min(v)

    def med(name):
        return float(np.median([r[name] for r in rounds]))

    s_tx, s_rx = spread("tx_emit"), spread("rx_ingest")
    line = {
        "workload": "datamsg", "codec": "RS8", "k": k, "m": m, "blocks": nb, "vec": vec, "seg_stride": vec,
        "segments_per_block": a.sent, "messages": count, "fec_id": fec_id, "header_bytes": H, "fti": True,
        "first_block_id": a.first_block_id, "message_bytes": nbytes, "copy_bytes": copy_bytes,
        "rounds": a.rounds, "iters": a.iters, "warmup": a.warmup,
        "ms_per_call": [{n: round(v, 4) for n, v in r.items()} for r in rounds],
        "tx_emit_data_vs_tx_emit": [round(r["tx_emit_data"] / r["tx_emit"], 4) for r in rounds],
        "rx_ingest_data_vs_rx_ingest": [round(r["rx_ingest_data"] / r["rx_ingest"], 4) for r in rounds],
        "tx_emit_spread": round(s_tx, 5), "rx_ingest_spread": round(s_rx, 5),
        "tx_emit_data_within_spread_plus_5pct": all(r["tx_emit_data"] <= r["tx_emit"] * (1.05 + s_tx) for r in rounds),
        "rx_ingest_data_within_spread_plus_5pct": all(r["rx_ingest_data"] <= r["rx_ingest"] * (1.05 + s_rx)
                                                      for r in rounds),
        "tx_emit_data_GBps": round(nbytes / (med("tx_emit_data") * 1e-3) / 1e9, 1),
        "rx_ingest_data_GBps": round(nbytes / (med("rx_ingest_data") * 1e-3) / 1e9, 1),
        "stream_copy_GBps": round(copy_bytes / (med("stream_copy") * 1e-3) / 1e9, 1),
        "tx_emit_data_rate_vs_stream_copy": round((nbytes / med("tx_emit_data")) / (copy_bytes / med("stream_copy")), 3),
        "rx_ingest_data_rate_vs_stream_copy": round((nbytes / med("rx_ingest_data")) / (copy_bytes / med("stream_copy")),
                                                    3),
        "rate_note": "GB/s = message bytes written (read) per second; the payload bytes are read (written) once more",
        "every_entry_emitted": emitted_ok, "same_payloads_and_ids_as_tx_emit": same_payloads and same_ids,
        "device_parse_equals_the_list": parsed_ok, "every_datagram_placed": placed_ok,
        "same_bytes_as_rx_ingest": same,
    }
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    if not (emitted_ok and same_payloads and same_ids and parsed_ok and placed_ok and same):
        raise SystemExit("bench_datamsg: the new calls wrote, parsed or placed other bytes than the parent calls")


if __name__ == "__main__":
    main()
