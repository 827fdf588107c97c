"""Object segmentation on the device against the parent's route to the same bytes and the streaming copy.

Per shape and direction three candidates move the same bytes:
  (a) the new call: nfec_object_read / nfec_object_write;
  (b) the assembly call that reaches the same bytes without them: for read, nfec_rx_place with one
      identity descriptor per source segment (built beforehand; the reception mask is re-zeroed ahead
      of every call, outside the timed region); for write, nfec_tx_emit with fec_id 0, gap 0 and the
      object's offsets;
  (c) nfec_util_stream_copy of the same byte count.
They alternate a, b, c in `--rounds` rounds; every candidate of a round is timed with HIP events
around each of `--iters` calls (the sum is the round's figure) after `--warmup` untimed calls.  The
requirement: in every round (a) takes no longer than (b).  The ratio to (c) is recorded only.

Shapes: RS8(64,32), 65,536 blocks; segment_size 1,392 / vector 1,400 / seg_stride 1,400 with the
object 16-byte aligned, and 1,452 / 1,460 / 1,464 with the object's base 1 byte past a 16-byte
boundary.  The object is blocks * 64 * segment_size - 700 bytes, so its final segment is short.

One JSON line per (shape, direction) is appended to --out (default profiles/r15/obj/obj.jsonl) and
printed.  A run without a GPU fails.

  python3 tools/bench_obj.py
  rocprofv3 --pmc FETCH_SIZE --output-format csv -d OUT/p0 -o pmc -- python3 tools/bench_obj.py --pmc-run
  rocprofv3 --pmc WRITE_SIZE --output-format csv -d OUT/p1 -o pmc -- python3 tools/bench_obj.py --pmc-run
  python3 tools/parse_pmc.py OUT        (counters in a run of their own, one per pass, no tracing)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [
    # segment_size, vector, seg_stride, object base modulo 16
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
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "obj", "obj.jsonl"))
    p.add_argument("--pmc-run", action="store_true",
                   help="two calls of each new kernel and of the copy per shape, nothing timed: the "
                        "workload of a rocprofv3 --pmc pass")
    a = p.parse_args()

    import numpy as np
    import torch
    import norm_amd as na

    if not torch.cuda.is_available() or na.device_count() < 1:
        raise SystemExit("bench_obj: needs an MI355X")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    k, m, nb = a.k, a.m, a.blocks
    results = []
    for seg, vec, stride, base in SHAPES:
        size = nb * k * seg - 700
        lay = na.object_layout(size, seg, k)
        assert lay.num_blocks == nb
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
        obj = src_buf[base:base + size]
        out_a = out_buf[base:base + size]
        out_b = alt_buf[base:base + size]
        batch_a = torch.empty((nb, k + m, stride), dtype=torch.uint8, device="cuda")
        batch_b = torch.empty_like(batch_a)
        batch_a.fill_(0x5A)
        batch_b.fill_(0x5A)
        # identity descriptors: segment g of the object, in (block, segment) order, starts at g * segment_size
        nseg = lay.num_segments
        g = torch.arange(nseg, dtype=torch.int64, device="cuda")
        big = lay.large_block_count * lay.large_block_size
        rest = (g - big).clamp_(min=0)
        blk = torch.where(g < big, g // max(lay.large_block_size, 1),
                          lay.large_block_count + rest // lay.small_block_size)
        sym = torch.where(g < big, g % max(lay.large_block_size, 1), rest % lay.small_block_size)
        offsets = g * seg
        length = torch.full((nseg,), seg, dtype=torch.int16, device="cuda")
        length[nseg - 1] = lay.final_segment_size
        block_index, symbol_id = blk.to(torch.int32), sym.to(torch.int16)
        del g, rest, blk, sym
        dnd = torch.from_numpy(na.object_block_sizes(lay, 0, nb).view(np.int16)).cuda()
        mask = na.received_mask(nb, k, m)
        copy_bytes = (size + pad) & ~15
        csrc, cdst = src_buf[:copy_bytes], out_buf[:copy_bytes]

        cands = {
            "read": [
                ("object_read", lambda: enc.read_object(obj, lay, batch_a, stream=stream), None),
                ("rx_place", lambda: enc.place_segments(batch_b, mask, obj, offsets, block_index, symbol_id, length,
                                                        num_data=dnd, stream=stream), lambda: mask.zero_()),
                ("stream_copy", lambda: na.stream_copy(cdst, csrc, stream=stream), None),
            ],
            "write": [
                ("object_write", lambda: enc.write_object(out_a, lay, batch_a, stream=stream), None),
                ("tx_emit", lambda: enc.emit_segments(batch_a, out_b, offsets, block_index, symbol_id, length,
                                                      fec_id=0, num_data=dnd, stream=stream), None),
                ("stream_copy", lambda: na.stream_copy(cdst, csrc, stream=stream), None),
            ],
        }

        if a.pmc_run:
            for direction in ("read", "write"):
                for name, fn, before in cands[direction]:
                    if name in ("rx_place", "tx_emit"):
                        continue
                    for _ in range(2):
                        fn()
            torch.cuda.synchronize()
            continue

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

        for direction in ("read", "write"):
            rounds = []
            for _ in range(a.rounds):
                rounds.append({name: timed(fn, before) for name, fn, before in cands[direction]})
            new, old = cands[direction][0][0], cands[direction][1][0]
            # both routes wrote the same bytes
            if direction == "read":
                same = all(bool(torch.equal(batch_a[b0:b0 + 4096, :k, :vec], batch_b[b0:b0 + 4096, :k, :vec]))
                           for b0 in range(0, nb, 4096))
            else:
                same = bool(torch.equal(out_a, out_b))
            a_ms = float(np.median([r[new] for r in rounds]))
            c_ms = float(np.median([r["stream_copy"] for r in rounds]))
            line = {
                "workload": "obj", "direction": direction, "codec": "RS8", "k": k, "m": m, "blocks": nb,
                "segment_size": seg, "vec": vec, "seg_stride": stride, "object_base_mod16": base,
                "object_bytes": size, "copy_bytes": copy_bytes, "rounds": a.rounds, "iters": a.iters, "warmup": a.warmup,
                "ms_per_call": [{n: round(v, 4) for n, v in r.items()} for r in rounds],
                "new": new, "parent_route": old,
                "new_vs_parent_route": [round(r[new] / r[old], 4) for r in rounds],
                "new_no_slower_in_every_round": all(r[new] <= r[old] for r in rounds),
                "new_GBps": round(size / (a_ms * 1e-3) / 1e9, 1),
                "stream_copy_GBps": round(copy_bytes / (c_ms * 1e-3) / 1e9, 1),
                "new_rate_vs_stream_copy": round((size / a_ms) / (copy_bytes / c_ms), 3),
                "rate_note": "GB/s = object bytes moved (or bytes copied) per second, each byte read once and written once",
                "same_bytes_as_parent_route": same,
            }
            results.append(line)
            print(json.dumps(line), flush=True)
        del src_buf, out_buf, alt_buf, batch_a, batch_b, obj, out_a, out_b, csrc, cdst
        torch.cuda.empty_cache()
    if results:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in results:
                f.write(json.dumps(line) + "\n")
        if not all(r["new_no_slower_in_every_round"] and r["same_bytes_as_parent_route"] for r in results):
            raise SystemExit("bench_obj: a new call was slower than the parent's route in some round, or wrote other bytes")


if __name__ == "__main__":
    main()
