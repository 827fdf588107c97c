"""Sender repair state on the device against the receiver's step that wrote the NACKs.

nfec_tx_handle_nacks reads the bytes nfec_rx_repair_requests writes, so that call over the same
blocks is the yardstick: per population the calls alternate in `--rounds` rounds, each timed with HIP
events around each of `--iters` calls after `--warmup` untimed ones.  The content is what
nfec_rx_repair_requests_host produces for a reception mask of tools/bench_nack.py's populations, cut
into NACK messages of at most 1,400 bytes at request boundaries; the handle call starts from TxInit's
state every time (a memset of the state, timed separately and subtracted nowhere), the activation from
the state the handle call leaves, the end-of-block step from empty pending masks.  All buffers are
allocated once and the calls go through the C ABI, so no allocation is timed.

Shape: RS8(64,32), 65,536 blocks.  Populations:
  loss40   every segment lost with probability 0.40
  absent5  loss 0.40 and 5 % of the blocks without a received segment, in runs
One JSON line per population is appended to --out and printed: the times, the totals, and whether the
device state equals the host entries' (required).  A run without a GPU fails.

  python3 tools/bench_txrepair.py
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
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "txrepair", "txrepair.jsonl"))
    a = p.parse_args()

    import numpy as np
    import torch
    import norm_amd as na
    from norm_amd import _native as N

    if not torch.cuda.is_available() or na.device_count() < 1:
        raise SystemExit("bench_txrepair: needs an MI355X")
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
        h_state = na.tx_repair_state(nb, k, m, 0)
        want_totals = na.tx_handle_nacks_host(k, m, h_state, content, off, ln, None, 5, 8, 1, 0)
        handled = h_state.clone()
        h_pending = np.zeros((nb, words), np.uint32)
        want_act = na.tx_activate_repairs_host(k, m, h_state, h_pending)
        units = int(want_totals[0])

        dmask = torch.from_numpy(mask.view(np.int32)).cuda()
        d_content = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")
        rows = torch.zeros((nb + 1, 2), dtype=torch.int64, device="cuda")
        rtotals = torch.zeros(4, dtype=torch.int64, device="cuda")
        wire = torch.from_numpy(content.copy()).cuda()
        d_off, d_ln = torch.from_numpy(off.view(np.int64)).cuda(), torch.from_numpy(ln.view(np.int16)).cuda()
        state = na.tx_repair_state(nb, k, m, 0, device="cuda")
        pending = torch.zeros((nb, words), dtype=torch.int32, device="cuda")
        ws = torch.zeros(int(L.nfec_tx_nack_workspace_bytes(units, off.size, nb)), dtype=torch.uint8, device="cuda")
        totals = torch.zeros(6, dtype=torch.int64, device="cuda")
        atotals = torch.zeros(3, dtype=torch.int64, device="cuda")
        st = state.struct()
        msg = N.RxMessages()
        msg.payloads, msg.payload_bytes = wire.data_ptr(), nbytes
        msg.offsets, msg.length, msg.count, msg.count_dev = d_off.data_ptr(), d_ln.data_ptr(), off.size, None

        def reset():
            for t in state.arrays():
                t.zero_()
            pending.zero_()

        def requests():
            N.check(L.nfec_rx_repair_requests(h, dmask.data_ptr(), words, None, nb, 5, 8, 1, 0, 0, max_units,
                                              d_content.data_ptr(), nbytes + 64, rows.data_ptr(), rtotals.data_ptr(), sp),
                    "nfec_rx_repair_requests")

        def handle():
            N.check(L.nfec_tx_handle_nacks(h, ctypes.byref(msg), 5, 8, 1, 0, None, nb, words, 0, ctypes.byref(st), units,
                                           ws.data_ptr(), ws.numel(), totals.data_ptr(), sp), "nfec_tx_handle_nacks")

        def activate():
            N.check(L.nfec_tx_activate_repairs(h, None, nb, 0, pending.data_ptr(), words, ctypes.byref(st),
                                               atotals.data_ptr(), sp), "nfec_tx_activate_repairs")

        def end_blocks():
            N.check(L.nfec_tx_end_blocks(h, None, nb, pending.data_ptr(), words, ctypes.byref(st), sp), "nfec_tx_end_blocks")

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

        def handled_state():  # the state a handle call leaves, for the activation to start from
            reset()
            handle()

        rounds, same = [], True
        for _ in range(a.rounds):
            r = {"repair_requests": timed(requests), "handle_nacks": timed(handle, reset)}
            torch.cuda.synchronize()
            got = state.to_host()
            same &= all(np.array_equal(x, y) for x, y in zip(got.arrays(), handled.arrays()))
            same &= np.array_equal(totals.cpu().numpy().view(np.uint64), want_totals)
            r["activate_repairs"] = timed(activate, handled_state)
            torch.cuda.synchronize()
            got = state.to_host()
            same &= all(np.array_equal(x, y) for x, y in zip(got.arrays(), h_state.arrays()))
            same &= np.array_equal(pending.cpu().numpy().view(np.uint32), h_pending)
            same &= np.array_equal(atotals.cpu().numpy().view(np.uint64), want_act)
            r["end_blocks"] = timed(end_blocks, pending.zero_)
            rounds.append(r)
        med = {n: float(np.median([r[n] for r in rounds])) for n in rounds[0]}
        line = dict(workload="txrepair", population=name, codec="RS8", k=k, m=m, blocks=nb, rounds=a.rounds, iters=a.iters,
                    warmup=a.warmup, ms_per_call=[{n: round(v, 4) for n, v in r.items()} for r in rounds],
                    median_ms={n: round(v, 4) for n, v in med.items()},
                    handle_vs_repair_requests=[round(r["handle_nacks"] / r["repair_requests"], 3) for r in rounds],
                    content_bytes=nbytes, messages=int(off.size), units=units, applied=int(want_totals[1]),
                    not_applied=int(want_totals[2]), block_bits=int(want_totals[3]), blocks_reset=int(want_act[0]),
                    blocks_activated=int(want_act[1]), pending_bits=int(want_act[2]), same_state_as_host_entries=bool(same))
        results.append(line)
        print(json.dumps(line), flush=True)
        del dmask, d_content, rows, wire, state, pending, ws
        torch.cuda.empty_cache()

    if results:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in results:
                f.write(json.dumps(line) + "\n")
        if not all(r["same_state_as_host_entries"] for r in results):
            raise SystemExit("bench_txrepair: the device state differs from the host entries'")


if __name__ == "__main__":
    main()
