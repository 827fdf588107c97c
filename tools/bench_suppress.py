"""NACK suppression and repair advertisements on the device against the calls they stand beside.

Three entries, each beside its yardstick in the same job, alternating in `--rounds` rounds, each call
timed with HIP events around each of `--iters` calls after `--warmup` untimed ones:
  nfec_rx_handle_repair_content   beside nfec_tx_handle_nacks: both read the same NACK messages
  nfec_rx_repair_pending          beside nfec_rx_repair_requests: both classify the same reception mask
  nfec_tx_repair_adv              beside nfec_rx_repair_requests: the same kernels over another mask
The populations and the content are tools/bench_txrepair.py's: the repair-request content
nfec_rx_repair_requests_host produces for a reception mask, cut into NACK messages of at most 1,400
bytes at request boundaries.  The receiver that overhears them has the same reception mask (every
SEGMENT-level unit is applied, the most work the handler can have) and starts from a zeroed state
every time (the memset is not timed); the decision runs on the state the handler leaves, the
advertisement on the sender's state behind nfec_tx_handle_nacks of the same messages.  All buffers are
allocated once and the calls go through the C ABI, so no allocation is timed.

Shape: RS8(64,32), 65,536 blocks.  Populations:
  loss40   every segment lost with probability 0.40
  absent5  loss 0.40 and 5 % of the blocks without a received segment, in runs
One JSON line per population is appended to --out and printed: the times, the totals, and whether the
device results equal the host entries' (required).  A run without a GPU fails.

  python3 tools/bench_suppress.py
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def split_messages(content, limit):
    """(offsets, lengths) of messages of at most `limit` bytes that end at request boundaries"""
    import numpy as np

    off, ln, at, start = [], [], 0, 0
    while at < len(content):
        size = 4 + (int(content[at + 2]) << 8 | int(content[at + 3]))
        if at + size - start > limit:
            off.append(start), ln.append(at - start)
            start = at
        at += size
    if at > start:
        off.append(start), ln.append(at - start)
    return np.array(off, np.uint64), np.array(ln, np.uint16)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--blocks", type=int, default=65536)
    p.add_argument("--k", type=int, default=64)
    p.add_argument("--m", type=int, default=32)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--only", default=None, help="one population (for a profiler run)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "suppress", "suppress.jsonl"))
    a = p.parse_args()

    import numpy as np
    import torch
    import norm_amd as na
    from norm_amd import _native as N

    if not torch.cuda.is_available() or na.device_count() < 1:
        raise SystemExit("bench_suppress: needs an MI355X")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    k, m, nb = a.k, a.m, a.blocks
    words = (k + m + 31) // 32
    enc = na.NormEncoderRS8()
    assert enc.Init(k, m, 1400)
    rng = np.random.default_rng(0x4E41434B)
    L = N.lib()
    h = enc._h
    sp = ctypes.c_void_p(stream.cuda_stream)
    max_units = (1400 - 4) // 16

    def population(loss, absent=0.0):
        got = rng.random((nb, words * 32)) >= loss
        if absent:
            run = 0
            for b in range(nb):  # runs of 1 to 6 absent blocks
                if run == 0 and rng.random() < absent / 3.5:
                    run = int(rng.integers(1, 7))
                if run:
                    got[b] = False
                    run -= 1
        got[:, k + m:] = False
        return np.packbits(got.reshape(nb, words, 32), axis=2, bitorder="little").view(np.uint32).reshape(nb, words)

    results = []
    for name, kw in (("loss40", dict(loss=0.40)), ("absent5", dict(loss=0.40, absent=0.05))):
        if a.only and a.only != name:
            continue
        mask = population(**kw)
        h_content, _, h_totals = na.rx_repair_requests_host(k, m, mask, None, 5, 8, 1, 0, 0, max_units)
        nbytes = int(h_totals[0])
        content = h_content[:nbytes]
        off, ln = split_messages(content, 1400)
        # the host entries: what the device has to leave
        h_rx = na.rx_repair_state(nb, k, m)
        want_handle = na.rx_handle_repair_content_host(k, m, h_rx, mask, content, off, ln, None, 5, 8, 1, 0)
        want_pending, want_words = na.rx_repair_pending_host(k, m, h_rx, mask)
        h_tx = na.tx_repair_state(nb, k, m, 0)
        tx_totals = na.tx_handle_nacks_host(k, m, h_tx, content, off, ln, None, 5, 8, 1, 0)
        want_adv, want_rows, want_adv_totals = na.tx_repair_adv_host(k, m, h_tx, None, 5, 8, 1, 0, max_units)
        adv_bytes = int(want_adv_totals[0])
        units = int(tx_totals[0])

        dmask = torch.from_numpy(mask.view(np.int32)).cuda()
        d_content = torch.zeros(max(nbytes, adv_bytes) + 64, dtype=torch.uint8, device="cuda")
        rows = torch.zeros((nb + 1, 2), dtype=torch.int64, device="cuda")
        rtotals = torch.zeros(4, dtype=torch.int64, device="cuda")
        wire = torch.from_numpy(content.copy()).cuda()
        d_off, d_ln = torch.from_numpy(off.view(np.int64)).cuda(), torch.from_numpy(ln.view(np.int16)).cuda()
        rx = na.rx_repair_state(nb, k, m, device="cuda")
        tx = na.tx_repair_state(nb, k, m, 0, device="cuda")
        ws = torch.zeros(int(L.nfec_tx_nack_workspace_bytes(units, off.size, nb)), dtype=torch.uint8, device="cuda")
        totals = torch.zeros(6, dtype=torch.int64, device="cuda")
        ttotals = torch.zeros(6, dtype=torch.int64, device="cuda")
        ptotals = torch.zeros(4, dtype=torch.int64, device="cuda")
        pwords = torch.zeros((nb + 31) // 32, dtype=torch.int32, device="cuda")
        rst, tst = rx.struct(), tx.struct()
        msg = N.RxMessages()
        msg.payloads, msg.payload_bytes = wire.data_ptr(), nbytes
        msg.offsets, msg.length, msg.count, msg.count_dev = d_off.data_ptr(), d_ln.data_ptr(), off.size, None
        cap = d_content.numel()

        def reset_rx():
            rx.zero()

        def reset_tx():
            for t in tx.arrays():
                t.zero_()

        def requests():
            N.check(L.nfec_rx_repair_requests(h, dmask.data_ptr(), words, None, nb, 5, 8, 1, 0, 0, max_units,
                                              d_content.data_ptr(), cap, rows.data_ptr(), rtotals.data_ptr(), sp),
                    "nfec_rx_repair_requests")

        def handle_nacks():
            N.check(L.nfec_tx_handle_nacks(h, ctypes.byref(msg), 5, 8, 1, 0, None, nb, words, 0, ctypes.byref(tst), units,
                                           ws.data_ptr(), ws.numel(), ttotals.data_ptr(), sp), "nfec_tx_handle_nacks")

        def handle_content():
            N.check(L.nfec_rx_handle_repair_content(h, ctypes.byref(msg), 5, 8, 1, 0, dmask.data_ptr(), words, None, nb,
                                                    ctypes.byref(rst), totals.data_ptr(), sp), "nfec_rx_handle_repair_content")

        def pending():
            N.check(L.nfec_rx_repair_pending(h, dmask.data_ptr(), words, None, nb, ctypes.byref(rst), 0, pwords.data_ptr(),
                                             ptotals.data_ptr(), sp), "nfec_rx_repair_pending")

        def adv():
            N.check(L.nfec_tx_repair_adv(h, ctypes.byref(tst), words, None, nb, 5, 8, 1, 0, max_units, d_content.data_ptr(),
                                         cap, rows.data_ptr(), rtotals.data_ptr(), sp), "nfec_tx_repair_adv")

        def timed(fn, before=None):
            total = 0.0
            for i in range(a.warmup + a.iters):
                if before:
                    before()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                total += e0.elapsed_time(e1) if i >= a.warmup else 0.0
            return total / a.iters

        rounds, same = [], True
        for _ in range(a.rounds):
            r = {"handle_nacks": timed(handle_nacks, reset_tx), "handle_repair_content": timed(handle_content, reset_rx)}
            torch.cuda.synchronize()
            same &= all(np.array_equal(x, y) for x, y in zip(rx.to_host().arrays(), h_rx.arrays()))
            same &= np.array_equal(totals.cpu().numpy().view(np.uint64), want_handle)
            r["repair_requests"] = timed(requests)
            r["repair_pending"] = timed(pending)  # on the state the handler left
            torch.cuda.synchronize()
            same &= np.array_equal(ptotals.cpu().numpy().view(np.uint64), want_pending)
            same &= np.array_equal(pwords.cpu().numpy().view(np.uint32), want_words)
            r["repair_requests_2"] = timed(requests)
            r["repair_adv"] = timed(adv)  # on the state the last handle_nacks left
            torch.cuda.synchronize()
            same &= np.array_equal(rtotals.cpu().numpy().view(np.uint64), want_adv_totals)
            same &= np.array_equal(d_content.cpu().numpy()[:adv_bytes], want_adv[:adv_bytes])
            same &= np.array_equal(rows.cpu().numpy().view(np.uint64), want_rows)
            rounds.append(r)
        med = {n: float(np.median([r[n] for r in rounds])) for n in rounds[0]}
        line = dict(workload="suppress", population=name, codec="RS8", k=k, m=m, blocks=nb, rounds=a.rounds, iters=a.iters,
                    warmup=a.warmup, ms_per_call=[{n: round(v, 4) for n, v in r.items()} for r in rounds],
                    median_ms={n: round(v, 4) for n, v in med.items()},
                    handle_content_vs_handle_nacks=[round(r["handle_repair_content"] / r["handle_nacks"], 3) for r in rounds],
                    pending_vs_repair_requests=[round(r["repair_pending"] / r["repair_requests"], 3) for r in rounds],
                    adv_vs_repair_requests=[round(r["repair_adv"] / r["repair_requests_2"], 3) for r in rounds],
                    content_bytes=nbytes, messages=int(off.size), units=units, applied=int(want_handle[1]),
                    not_applied=int(want_handle[2]), block_bits=int(want_handle[3]), send=int(want_pending[0]),
                    blocks_pending=int(want_pending[1]), needing_suppressed=int(want_pending[2]),
                    absent_suppressed=int(want_pending[3]), adv_bytes=adv_bytes, adv_requests=int(want_adv_totals[1]),
                    adv_segment_blocks=int(want_adv_totals[2]), adv_whole_blocks=int(want_adv_totals[3]),
                    same_as_host_entries=bool(same))
        results.append(line)
        print(json.dumps(line), flush=True)
        del dmask, d_content, rows, wire, rx, tx, ws
        torch.cuda.empty_cache()

    if results:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in results:
                f.write(json.dumps(line) + "\n")
        if not all(r["same_as_host_entries"] for r in results):
            raise SystemExit("bench_suppress: the device results differ from the host entries'")


if __name__ == "__main__":
    main()
