"""The receiver intake against the parent's route to the same bytes and the streaming copy.

Three candidates place the same messages from the same wire buffer:
  (a) the new call: nfec_rx_ingest, which reads each message's FEC payload ID on the device;
  (b) nfec_rx_place on (block, symbol) descriptors parsed beforehand: the parent's route with its
      host hop (download the IDs, nfec_payload_id_read, upload two arrays) not charged;
  (c) nfec_util_stream_copy of the payload byte count.
They alternate a, b, c in `--rounds` rounds; every candidate of a round is timed with HIP events
around each of `--iters` calls (the mean is the round's figure) after `--warmup` untimed calls.  The
reception mask is re-zeroed ahead of every call of (a) and (b), outside the timed region.  Beside
them each round times (a) and (b) once more on the mask their last call left full: every message
is then a duplicate, which costs the descriptor chain, the ID fetch and the claim, and no copy.

The requirement: in every round (a) takes no longer than (b) * (1 + s), s the largest relative
difference between (b)'s own rounds of this run.  Only a comparison inside one run counts (DESIGN
9, item 11).  The ratio to (c) is recorded only.

Shape (profiles/r09/rx/): RS8(64, 32), 1,400-byte vectors, 65,536 blocks, 80 of 96 segments of
every block in an order shuffled over the batch, fec_id 5, 13 free bytes in front of every payload
(so every payload alignment occurs).  The wire buffer is written once by nfec_tx_list + nfec_tx_emit.

One JSON line is appended to --out (default profiles/r16/rx_ingest/ingest.jsonl) and printed.  A run
without a GPU fails.

  python3 tools/bench_rx_ingest.py
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
    p.add_argument("--sent", type=int, default=80, help="segments of every block that arrive")
    p.add_argument("--gap", type=int, default=13)
    p.add_argument("--first-block-id", type=lambda s: int(s, 0), default=0xFFF000,
                   help="the window wraps fec_id 5's 24-bit block field inside the batch")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "rx_ingest", "ingest.jsonl"))
    a = p.parse_args()

    import numpy as np
    import torch
    import norm_amd as na

    if not torch.cuda.is_available() or na.device_count() < 1:
        raise SystemExit("bench_rx_ingest: needs an MI355X")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    k, m, nb, vec = a.k, a.m, a.blocks, a.vec
    fec_id, fec_m = 5, 8
    enc = na.NormEncoderRS8()
    assert enc.Init(k, m, vec)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0x4E4F524D)

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
    nbytes = count * (a.gap + vec)
    wire = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")
    off, blk, sym, ln, start = enc.list_pending(pending, gap=a.gap, capacity=count)
    enc.emit_segments(sent, wire, off, blk, sym, ln, count_dev=start[nb, :1], fec_id=fec_id, fec_m=fec_m,
                      first_block_id=a.first_block_id)
    torch.cuda.synchronize()
    assert start[nb].tolist() == [count, nbytes], start[nb].tolist()
    # arrival order: shuffled over the whole batch
    order = torch.randperm(count, device="cuda", generator=gen)
    off, ln, want_blk, want_sym = off[order].contiguous(), ln[order].contiguous(), blk[order], sym[order]
    del order, blk, sym, pending

    batch_a = torch.empty_like(sent)
    batch_b = torch.empty_like(sent)
    batch_a.fill_(0x5A)
    batch_b.fill_(0x5A)
    mask_a, mask_b = na.received_mask(nb, k, m), na.received_mask(nb, k, m)
    # (b)'s descriptors, parsed beforehand: here by an untimed intake call, checked against the list
    block_index = torch.empty(count, dtype=torch.int32, device="cuda")
    symbol_id = torch.empty(count, dtype=torch.int16, device="cuda")
    stats = torch.zeros(3, dtype=torch.int32, device="cuda")
    enc.ingest_messages(batch_a, mask_a, wire, off, ln, fec_id, fec_m, first_block_id=a.first_block_id,
                        block_index_out=block_index, symbol_id_out=symbol_id, stats=stats, stream=stream)
    torch.cuda.synchronize()
    parsed_ok = bool(torch.equal(block_index, want_blk)) and bool(torch.equal(symbol_id, want_sym))
    placed_ok = stats.tolist() == [count, 0, 0]
    del want_blk, want_sym

    copy_bytes = (count * vec) & ~15
    cdst = sent.view(-1)[:copy_bytes]  # the sender's batch has served its purpose
    csrc = wire[:copy_bytes]

    def ingest():
        enc.ingest_messages(batch_a, mask_a, wire, off, ln, fec_id, fec_m, first_block_id=a.first_block_id,
                            stream=stream)

    def place():
        enc.place_segments(batch_b, mask_b, wire, off, block_index, symbol_id, ln, stream=stream)

    cands = [
        ("rx_ingest", ingest, lambda: mask_a.zero_()),
        ("rx_place", place, lambda: mask_b.zero_()),
        ("stream_copy", lambda: na.stream_copy(cdst, csrc, stream=stream), None),
        ("rx_ingest_all_duplicates", ingest, None),  # the masks are full from the calls above
        ("rx_place_all_duplicates", place, None),
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
    b_ms = [r["rx_place"] for r in rounds]
    spread = (max(b_ms) - min(b_ms)) / min(b_ms)
    a_ms = float(np.median([r["rx_ingest"] for r in rounds]))
    c_ms = float(np.median([r["stream_copy"] for r in rounds]))
    payload = count * vec
    line = {
        "workload": "rx_ingest", "codec": "RS8", "k": k, "m": m, "blocks": nb, "vec": vec, "seg_stride": vec,
        "segments_per_block": a.sent, "messages": count, "fec_id": fec_id, "gap": a.gap,
        "first_block_id": a.first_block_id, "payload_bytes": payload, "copy_bytes": copy_bytes,
        "rounds": a.rounds, "iters": a.iters, "warmup": a.warmup,
        "ms_per_call": [{n: round(v, 4) for n, v in r.items()} for r in rounds],
        "new": "rx_ingest", "parent_route": "rx_place",
        "new_vs_parent_route": [round(r["rx_ingest"] / r["rx_place"], 4) for r in rounds],
        "parent_route_spread": round(spread, 5),
        "new_within_spread_in_every_round": all(r["rx_ingest"] <= r["rx_place"] * (1 + spread) for r in rounds),
        "all_duplicates_new_vs_parent_route": [round(r["rx_ingest_all_duplicates"] / r["rx_place_all_duplicates"], 4)
                                               for r in rounds],
        "new_GBps": round(payload / (a_ms * 1e-3) / 1e9, 1),
        "stream_copy_GBps": round(copy_bytes / (c_ms * 1e-3) / 1e9, 1),
        "new_rate_vs_stream_copy": round((payload / a_ms) / (copy_bytes / c_ms), 3),
        "rate_note": "GB/s = payload bytes placed (or bytes copied) per second, each byte read once and written once",
        "device_parse_equals_the_list": parsed_ok, "every_message_placed": placed_ok,
        "same_bytes_as_parent_route": same,
    }
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    if not (parsed_ok and placed_ok and same):
        raise SystemExit("bench_rx_ingest: the intake parsed or placed other bytes than the parent's route")
    if not line["new_within_spread_in_every_round"]:
        raise SystemExit("bench_rx_ingest: nfec_rx_ingest was slower than nfec_rx_place beyond its spread in some round")


if __name__ == "__main__":
    main()
