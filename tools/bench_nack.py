"""Repair requests on the device against the transmission list over the same words.

nfec_rx_repair_requests and nfec_tx_list both count, scan and expand the words of a per-block mask,
so the list is the yardstick: per mask population the two calls alternate in `--rounds` rounds, each
timed with HIP events around each of `--iters` calls after `--warmup` untimed ones.  The list takes the
words as pending masks (every set bit an entry), the new call as reception masks (every clear bit a
candidate).  Both write into buffers allocated once, through the C ABI, so no allocation is timed.

Shape: RS8(64,32), 65,536 blocks.  Populations:
  loss40   every segment lost with probability 0.40 (mostly e <= m: parity requests)
  loss65   ... 0.65 (mostly e > m: explicit requests)
  absent5  loss 0.40 and 5 % of the blocks without a received segment, in runs
  mixed_nd loss 0.40, num_data k or k - 1
One JSON line per population is appended to --out and printed: both times, their ratio, and whether
the new call's median is above the list's by more than the list's own spread between the rounds
(recorded, not required).  A run without a GPU fails.

  python3 tools/bench_nack.py
"""
import argparse
import ctypes
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
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--only", default=None, help="one population (for a profiler run)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "nack", "nack.jsonl"))
    a = p.parse_args()

    import numpy as np
    import torch
    import norm_amd as na
    from norm_amd import _native as N

    if not torch.cuda.is_available() or na.device_count() < 1:
        raise SystemExit("bench_nack: needs an MI355X")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    k, m, nb = a.k, a.m, a.blocks
    words = (k + m + 31) // 32
    dec = na.NormDecoderRS8()
    assert dec.Init(k, m, 1400)
    rng = np.random.default_rng(0x4E41434B)
    L = N.lib()
    h = dec._h
    sp = ctypes.c_void_p(stream.cuda_stream)

    def population(loss, absent=0.0, mixed=False):
        got = rng.random((nb, words * 32)) >= loss
        nd = np.full(nb, k, np.uint16)
        if mixed:
            nd[rng.random(nb) < 0.5] = k - 1
        if absent:
            run = 0
            for b in range(nb):  # runs of 1 to 6 absent blocks
                if run == 0 and rng.random() < absent / 3.5:
                    run = int(rng.integers(1, 7))
                if run:
                    got[b] = False
                    run -= 1
        got[:, k + m:] = False
        mask = np.packbits(got.reshape(nb, words, 32), axis=2, bitorder="little").view(np.uint32).reshape(nb, words)
        return mask, nd

    pops = [("loss40", dict(loss=0.40)), ("loss65", dict(loss=0.65)), ("absent5", dict(loss=0.40, absent=0.05)),
            ("mixed_nd", dict(loss=0.40, mixed=True))]
    results = []
    for name, kw in pops:
        if a.only and a.only != name:
            continue
        mask, nd = population(**kw)
        dmask = torch.from_numpy(mask.view(np.int32)).cuda()
        dnd = torch.from_numpy(nd.view(np.int16)).cuda()
        # the host entry sizes the buffers and is what the device has to produce
        h_content, h_start, h_totals = na.rx_repair_requests_host(k, m, mask, nd, 5, 8, 1, 0)
        cap = int(h_totals[0]) + 64
        content = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        rows = torch.zeros((nb + 1, 2), dtype=torch.int64, device="cuda")
        totals = torch.zeros(4, dtype=torch.int64, device="cuda")
        entries = int(np.unpackbits(mask.view(np.uint8)).sum())
        off = torch.zeros(entries, dtype=torch.int64, device="cuda")
        blk = torch.zeros(entries, dtype=torch.int32, device="cuda")
        sym = torch.zeros(entries, dtype=torch.int16, device="cuda")
        ln = torch.zeros(entries, dtype=torch.int16, device="cuda")
        lrows = torch.zeros((nb + 1, 2), dtype=torch.int64, device="cuda")

        def nack():
            N.check(L.nfec_rx_repair_requests(h, dmask.data_ptr(), words, dnd.data_ptr(), nb, 5, 8, 1, 0, 0,
                                              na.repair_max_units(5), content.data_ptr(), cap, rows.data_ptr(),
                                              totals.data_ptr(), sp), "nfec_rx_repair_requests")

        def tx_list():
            N.check(L.nfec_tx_list(h, dmask.data_ptr(), words, dnd.data_ptr(), nb, None, 0, 4, off.data_ptr(),
                                   blk.data_ptr(), sym.data_ptr(), ln.data_ptr(), entries, lrows.data_ptr(), sp),
                    "nfec_tx_list")

        def timed(fn):
            for _ in range(a.warmup):
                fn()
            total = 0.0
            for _ in range(a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                total += e0.elapsed_time(e1)
            return total / a.iters

        rounds = [{"repair_requests": timed(nack), "tx_list": timed(tx_list)} for _ in range(a.rounds)]
        torch.cuda.synchronize()
        same = (np.array_equal(totals.cpu().numpy().view(np.uint64), h_totals)
                and np.array_equal(content.cpu().numpy()[:cap - 64], h_content[:cap - 64])
                and np.array_equal(rows.cpu().numpy().view(np.uint64), h_start))
        med = {n: float(np.median([r[n] for r in rounds])) for n in rounds[0]}
        spread = max(r["tx_list"] for r in rounds) - min(r["tx_list"] for r in rounds)
        line = dict(workload="nack", population=name, codec="RS8", k=k, m=m, blocks=nb, rounds=a.rounds, iters=a.iters,
                    warmup=a.warmup, ms_per_call=[{n: round(v, 4) for n, v in r.items()} for r in rounds],
                    median_ms={n: round(v, 4) for n, v in med.items()},
                    new_vs_tx_list=[round(r["repair_requests"] / r["tx_list"], 3) for r in rounds],
                    tx_list_spread_ms=round(spread, 4), new_minus_tx_list_ms=round(med["repair_requests"] - med["tx_list"], 4),
                    new_above_tx_list_by_more_than_its_spread=bool(med["repair_requests"] - med["tx_list"] > spread),
                    content_bytes=int(h_totals[0]), requests=int(h_totals[1]), needing_blocks=int(h_totals[2]),
                    absent_blocks=int(h_totals[3]), tx_list_entries=entries, same_bytes_as_host_entry=bool(same))
        results.append(line)
        print(json.dumps(line), flush=True)
        del dmask, content, rows, totals, off, blk, sym, ln, lrows
        torch.cuda.empty_cache()

    if results:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in results:
                f.write(json.dumps(line) + "\n")
        if not all(r["same_bytes_as_host_entry"] for r in results):
            raise SystemExit("bench_nack: the device content differs from the host entry's")


if __name__ == "__main__":
    main()
