"""Stream pack / unpack on the device against the assembly calls that move the same bytes, and the frame call.

Per shape three candidates alternate in `--rounds` rounds, each timed with HIP events around each of
`--iters` calls after `--warmup` untimed ones:
  pack:   (a) nfec_stream_pack of full segments from a table; (b) nfec_rx_place fed one identity
          descriptor per segment over the same stream bytes (the reception mask is re-zeroed ahead of
          every call, outside the timed region); (c) nfec_util_stream_copy of the same byte count.
  unpack: (a) nfec_stream_unpack of the batch pack filled; (b) nfec_tx_emit with fec_id 0 at the
          stream's offsets; (c) the streaming copy.  A window addresses 2^32 bytes of stream at the
          most, so unpack and its comparators run over the first floor(2^32 / (k * segment_size))
          blocks when the batch holds more.
The requirement: the new call's median over the rounds is above the assembly call's by no more than
that call's own spread (max - min) between the rounds of this job.  Ratios to the object calls come
from profiles/r15/obj (same shapes); the ratio to (c) is recorded.

Then the frame call: blocks * k segments of segment_size bytes from 1,024-byte messages (every write
EOM, the last FLUSH), timed the same way.

Shapes: RS8(64,32), 65,536 blocks; segment_size 1,392 / vector 1,400 / seg_stride 1,400 with the
stream 16-byte aligned, and 1,452 / 1,460 / 1,464 with the stream's base 1 byte past a 16-byte
boundary.  One JSON line per measurement is appended to --out and printed.  A run without a GPU fails.

  python3 tools/bench_stream.py
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [
    # segment_size, vector, seg_stride, stream base modulo 16
    (1392, 1400, 1400, 0),
    (1452, 1460, 1464, 1),
]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--blocks", type=int, default=65536)
    p.add_argument("--k", type=int, default=64)
    p.add_argument("--m", type=int, default=32)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--message", type=int, default=1024, help="bytes per write of the frame measurement")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "stream", "stream.jsonl"))
    a = p.parse_args()

    import numpy as np
    import torch
    import norm_amd as na

    if not torch.cuda.is_available() or na.device_count() < 1:
        raise SystemExit("bench_stream: needs an MI355X")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    k, m, nb = a.k, a.m, a.blocks
    results = []

    def timed(fn, before=None):
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

    def compare(direction, cands, nbytes, copy_bytes, same, extra):
        rounds = [{name: timed(fn, before) for name, fn, before in cands} for _ in range(a.rounds)]
        new, old = cands[0][0], cands[1][0]
        med = {n: float(np.median([r[n] for r in rounds])) for n in rounds[0]}
        spread = max(r[old] for r in rounds) - min(r[old] for r in rounds)
        line = dict(extra, workload="stream", direction=direction, rounds=a.rounds, iters=a.iters, warmup=a.warmup,
                    ms_per_call=[{n: round(v, 4) for n, v in r.items()} for r in rounds], new=new, assembly_call=old,
                    new_vs_assembly=[round(r[new] / r[old], 4) for r in rounds],
                    median_ms={n: round(v, 4) for n, v in med.items()},
                    assembly_spread_ms=round(spread, 4), assembly_spread_rel=round(spread / med[old], 5),
                    new_minus_assembly_ms=round(med[new] - med[old], 4),
                    requirement_held=bool(med[new] - med[old] <= spread),
                    new_GBps=round(nbytes / (med[new] * 1e-3) / 1e9, 1),
                    stream_copy_GBps=round(copy_bytes / (med["stream_copy"] * 1e-3) / 1e9, 1),
                    new_rate_vs_stream_copy=round((nbytes / med[new]) / (copy_bytes / med["stream_copy"]), 3),
                    rate_note="GB/s = stream bytes moved (or bytes copied) per second, each byte read once and written once",
                    same_bytes_as_assembly_call=same())
        results.append(line)
        print(json.dumps(line), flush=True)

    for seg, vec, stride, base in SHAPES:
        nseg = nb * k
        size = nseg * seg
        enc = na.NormEncoderRS8()
        assert enc.Init(k, m, vec)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(0x4E4F524D)
        pad = (-size) % 16
        src_buf = torch.empty(16 + size + pad + 16, dtype=torch.uint8, device="cuda")
        for at in range(0, src_buf.numel(), 1 << 28):
            part = src_buf[at:at + (1 << 28)]
            part.copy_(torch.randint(0, 256, (part.numel(),), dtype=torch.uint8, device="cuda", generator=gen))
        out_buf = torch.empty_like(src_buf)
        alt_buf = torch.empty_like(src_buf)
        data = src_buf[base:base + size]
        batch_a = torch.empty((nb, k + m, stride), dtype=torch.uint8, device="cuda")
        batch_b = torch.empty_like(batch_a)
        batch_a.fill_(0x5A)
        batch_b.fill_(0x5A)
        g = torch.arange(nseg, dtype=torch.int64, device="cuda")
        seg_start = g * seg
        seg_len = torch.full((nseg,), seg, dtype=torch.int16, device="cuda")
        seg_ms = torch.zeros(nseg, dtype=torch.int16, device="cuda")
        block_index, symbol_id = (g // k).to(torch.int32), (g % k).to(torch.int16)
        del g
        mask = na.received_mask(nb, k, m)
        copy_bytes = (size + pad) & ~15
        shape = dict(codec="RS8", k=k, m=m, blocks=nb, segment_size=seg, vec=vec, seg_stride=stride, stream_base_mod16=base)

        compare("pack", [
            ("stream_pack", lambda: enc.pack_stream(data, seg_start, seg_len, seg_ms, batch_a, segment_size=seg,
                                                    stream=stream), None),
            ("rx_place", lambda: enc.place_segments(batch_b, mask, data, seg_start, block_index, symbol_id, seg_len,
                                                    stream=stream), lambda: mask.zero_()),
            ("stream_copy", lambda: na.stream_copy(out_buf[:copy_bytes], src_buf[:copy_bytes], stream=stream), None),
        ], size, copy_bytes,
            lambda: all(bool(torch.equal(batch_a[b0:b0 + 4096, :k, 8:8 + seg], batch_b[b0:b0 + 4096, :k, :seg]))
                        for b0 in range(0, nb, 4096)),
            dict(shape, stream_bytes=size, copy_bytes=copy_bytes))

        # unpack: the blocks one window can address
        nb_u = min(nb, (1 << 32) // (k * seg))
        size_u = nb_u * k * seg
        copy_u = size_u & ~15
        out_a, out_b = out_buf[base:base + size_u], alt_buf[base:base + size_u]
        n_u = nb_u * k
        # tx_emit sends a slot's first bytes: its comparator batch holds the payload from byte 0
        compare("unpack", [
            ("stream_unpack", lambda: enc.unpack_stream(batch_a[:nb_u], out_a, segment_size=seg, stream=stream), None),
            ("tx_emit", lambda: enc.emit_segments(batch_b[:nb_u], out_b, seg_start[:n_u], block_index[:n_u], symbol_id[:n_u],
                                                  seg_len[:n_u], fec_id=0, stream=stream), None),
            ("stream_copy", lambda: na.stream_copy(out_buf[:copy_u], src_buf[:copy_u], stream=stream), None),
        ], size_u, copy_u, lambda: bool(torch.equal(out_a, out_b)) and bool(torch.equal(out_a, data[:size_u])),
            dict(shape, blocks=nb_u, stream_bytes=size_u, copy_bytes=copy_u))
        del src_buf, out_buf, alt_buf, batch_a, batch_b, data, out_a, out_b, seg_start, seg_len, seg_ms, block_index, symbol_id
        torch.cuda.empty_cache()

        # frame: the same number of segments from --message byte writes
        n = size // a.message
        wl = torch.full((n,), a.message, dtype=torch.int32, device="cuda")
        wf = torch.full((n,), na.NFEC_STREAM_EOM, dtype=torch.uint8, device="cuda")
        wf[n - 1] = na.NFEC_STREAM_EOM | na.NFEC_STREAM_FLUSH
        want = -(-(n * a.message) // seg)
        out = {}

        def frame():
            out["r"] = enc.frame_stream(wl, wf, na.StreamState(), segment_size=seg, capacity=want, stream=stream)

        rounds = [timed(frame) for _ in range(a.rounds)]
        totals = out["r"][3].cpu().tolist()
        line = dict(shape, workload="stream", direction="frame", writes=n, message_bytes=a.message, segments=totals[0],
                    rounds=a.rounds, iters=a.iters, warmup=a.warmup, ms_per_call=[round(v, 4) for v in rounds],
                    median_ms=round(float(np.median(rounds)), 4),
                    segments_per_s=round(totals[0] / (float(np.median(rounds)) * 1e-3)),
                    note="includes the allocation of the call's tables and workspace by the Python wrapper",
                    totals_as_expected=bool(totals == [want, n * a.message, 0, 0]))
        results.append(line)
        print(json.dumps(line), flush=True)
        del wl, wf, out
        torch.cuda.empty_cache()

    if results:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in results:
                f.write(json.dumps(line) + "\n")
        bad = [r for r in results if r.get("requirement_held") is False or r.get("same_bytes_as_assembly_call") is False
               or r.get("totals_as_expected") is False]
        if bad:
            raise SystemExit("bench_stream: %d measurement(s) missed the requirement or moved other bytes" % len(bad))


if __name__ == "__main__":
    main()
