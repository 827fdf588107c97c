"""NORM_NACK and NORM_CMD(REPAIR_ADV) messages on the device against the host route they replace.

Timed in one job, alternating in `--rounds` rounds, with HIP events around each of `--iters` calls after
`--warmup` untimed ones:
  nfec_nack_fragment            with the producer's block_start as hint, and without it
  nfec_rx_ingest_control        on the datagrams the fragmenter wrote
  nfec_tx_repair_adv_message    on the same content
and beside them
  nfec_rx_repair_requests       the call that produces the content
  a device copy of the content's bytes
  the host route: the content to pinned host memory, nfec_nack_fragment_host, the messages back to the
  device, timed on the host's clock from the first copy's start to the last copy's end; the hinted device
  call is timed on the same clock too (launches and the wait for the stream), so the two compare.
The populations are tools/bench_suppress.py's; the content is nfec_rx_repair_requests' own for the
mask, requests as long as the wire allows (the fragmenter, not max_units, bounds a message).  S = 1400,
fec_id 5.  All buffers are allocated once and the calls go through the C ABI, so no allocation is timed.
Every timed output is compared once with the host twins'; `same_as_host_entries` goes into the line
and a difference fails the run.  One JSON line per population is appended to --out and printed.

  python3 tools/bench_ctlmsg.py
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--blocks", type=int, default=65536)
    p.add_argument("--k", type=int, default=64)
    p.add_argument("--m", type=int, default=32)
    p.add_argument("--segment-size", type=int, default=1400)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--only", default=None, help="one population (for a profiler run)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctlmsg", "ctlmsg.jsonl"))
    a = p.parse_args()

    import numpy as np
    import torch
    import norm_amd as na
    from norm_amd import _native as N

    if not torch.cuda.is_available() or na.device_count() < 1:
        raise SystemExit("bench_ctlmsg: needs an MI355X")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    k, m, nb, S = a.k, a.m, a.blocks, a.segment_size
    words = (k + m + 31) // 32
    enc = na.NormEncoderRS8()
    assert enc.Init(k, m, 1400)
    rng = np.random.default_rng(0x4E41434B)
    L = N.lib()
    h = enc._h
    sp = ctypes.c_void_p(stream.cuda_stream)
    max_units = na.repair_max_units(5)
    header = na.nack_header(0x0A000001, 0x0A0000FE, 7, grtt_response=(1, 2))
    adv_header = na.adv_header(0x0A0000FE, 7, sequence=1, grtt=0x40, backoff=4, gsize=1)
    H = na.nack_header_bytes(0)
    pitch = H + S

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
        cap = nbytes // (S - 32) + 8
        # the host twins: what the device has to leave
        want_wire, want_off, want_len, want_totals = na.nack_fragment_host(h_content[:nbytes], header, S, capacity=cap)
        messages = int(want_totals[0])
        f = na.ctl_filter(0x0A0000FE, 7, local_id=0x0A0000FE, flags=N.NFEC_CTL_TAKE_NACK)
        want_ctl = na.ctl_parse_host(f, want_wire, want_off[:messages], want_len[:messages])
        want_adv, want_adv_totals = na.adv_message_host(h_content[:nbytes], adv_header, S)

        dmask = torch.from_numpy(mask.view(np.int32)).cuda()
        d_content = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")
        d_copy = torch.zeros_like(d_content)
        rows = torch.zeros((nb + 1, 2), dtype=torch.int64, device="cuda")
        rtotals = torch.zeros(4, dtype=torch.int64, device="cuda")
        wire = torch.zeros(cap * pitch, dtype=torch.uint8, device="cuda")
        wire_host_route = torch.zeros_like(wire)
        d_off = torch.zeros(cap, dtype=torch.int64, device="cuda")
        d_len = torch.zeros(cap, dtype=torch.int16, device="cuda")
        ftotals = torch.zeros(6, dtype=torch.int64, device="cuda")
        ws = torch.zeros(int(L.nfec_nack_fragment_workspace_bytes(d_content.numel(), nb)), dtype=torch.uint8, device="cuda")
        c_cls = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        c_off = torch.zeros(cap, dtype=torch.int64, device="cuda")
        c_len = torch.zeros(cap, dtype=torch.int16, device="cuda")
        c_src = torch.zeros(cap, dtype=torch.int32, device="cuda")
        c_grtt = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
        c_stats = torch.zeros(9, dtype=torch.int32, device="cuda")
        adv_wire = torch.zeros(16 + S, dtype=torch.uint8, device="cuda")
        adv_len = torch.zeros(1, dtype=torch.int16, device="cuda")
        adv_totals = torch.zeros(3, dtype=torch.int64, device="cuda")
        pin_content = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
        pin_wire = torch.zeros(cap * pitch, dtype=torch.uint8).pin_memory()
        pin_off, pin_len, pin_totals = np.zeros(cap, np.uint64), np.zeros(cap, np.uint16), np.zeros(6, np.uint64)
        msg = N.RxMessages()
        msg.payloads, msg.payload_bytes = wire.data_ptr(), wire.numel()
        msg.offsets, msg.length, msg.count, msg.count_dev = d_off.data_ptr(), d_len.data_ptr(), cap, ftotals.data_ptr()

        def requests():
            N.check(L.nfec_rx_repair_requests(h, dmask.data_ptr(), words, None, nb, 5, 8, 1, 0, 0, max_units,
                                              d_content.data_ptr(), d_content.numel(), rows.data_ptr(), rtotals.data_ptr(), sp),
                    "nfec_rx_repair_requests")

        def fragment(hint):
            N.check(L.nfec_nack_fragment(h, d_content.data_ptr(), d_content.numel(), rtotals.data_ptr(),
                                         rows.data_ptr() if hint else None, nb if hint else 0, 5, S, ctypes.byref(header),
                                         wire.data_ptr(), wire.numel(), pitch, d_off.data_ptr(), d_len.data_ptr(), cap,
                                         ftotals.data_ptr(), ws.data_ptr(), ws.numel(), sp), "nfec_nack_fragment")

        def ingest():
            N.check(L.nfec_rx_ingest_control(h, ctypes.byref(msg), ctypes.byref(f), c_cls.data_ptr(), c_off.data_ptr(),
                                             c_len.data_ptr(), c_src.data_ptr(), c_grtt.data_ptr(), c_stats.data_ptr(), sp),
                    "nfec_rx_ingest_control")

        def adv():
            N.check(L.nfec_tx_repair_adv_message(h, d_content.data_ptr(), d_content.numel(), rtotals.data_ptr(), 5, S,
                                                 ctypes.byref(adv_header), adv_wire.data_ptr(), adv_wire.numel(),
                                                 adv_len.data_ptr(), adv_totals.data_ptr(), sp), "nfec_tx_repair_adv_message")

        def copy():
            d_copy[:nbytes].copy_(d_content[:nbytes])

        def host_route():
            pin_content.copy_(d_content[:nbytes], non_blocking=True)
            stream.synchronize()
            N.check(L.nfec_nack_fragment_host(pin_content.data_ptr(), nbytes, 5, S, ctypes.byref(header), pin_wire.data_ptr(),
                                              pin_wire.numel(), pitch, pin_off.ctypes.data, pin_len.ctypes.data, cap,
                                              pin_totals.ctypes.data), "nfec_nack_fragment_host")
            used = min(int(pin_totals[0]), cap) * pitch
            wire_host_route[:used].copy_(pin_wire[:used], non_blocking=True)
            stream.synchronize()

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

        def walled(fn):
            total = 0.0
            for i in range(a.warmup + a.iters):
                stream.synchronize()
                t0 = time.perf_counter()
                fn()
                stream.synchronize()
                total += (time.perf_counter() - t0) * 1e3 if i >= a.warmup else 0.0
            return total / a.iters

        def same_fragment():
            torch.cuda.synchronize()
            t = ftotals.cpu().numpy().view(np.uint64)
            ok = np.array_equal(t, want_totals)
            ok &= np.array_equal(d_off.cpu().numpy().view(np.uint64)[:messages], want_off[:messages])
            ok &= np.array_equal(d_len.cpu().numpy().view(np.uint16)[:messages], want_len[:messages])
            got = wire.cpu().numpy()
            for i in range(messages):
                o, n = int(want_off[i]), int(want_len[i])
                ok &= np.array_equal(got[o:o + n], want_wire[o:o + n])
            return bool(ok)

        requests()
        torch.cuda.synchronize()
        same = np.array_equal(d_content.cpu().numpy()[:nbytes], h_content[:nbytes])
        rounds = []
        for _ in range(a.rounds):
            r = {"repair_requests": timed(requests)}
            wire.zero_()
            r["nack_fragment_hint"] = timed(lambda: fragment(True))
            same &= same_fragment()
            r["ingest_control"] = timed(ingest, c_stats.zero_)
            torch.cuda.synchronize()
            got_ctl = (c_cls, c_off, c_len, c_src, c_grtt)
            for g, w, dt in zip(got_ctl, want_ctl, (np.uint8, np.uint64, np.uint16, np.uint32, np.uint32)):
                same &= np.array_equal(g.cpu().numpy().view(dt)[:messages], w)
            same &= np.array_equal(c_stats.cpu().numpy().view(np.uint32), want_ctl[5])
            wire.zero_()
            r["nack_fragment_no_hint"] = timed(lambda: fragment(False))
            same &= same_fragment()
            r["adv_message"] = timed(adv)
            torch.cuda.synchronize()
            n = int(adv_len.cpu().numpy().view(np.uint16)[0])
            same &= adv_wire.cpu().numpy()[:n].tobytes() == want_adv
            same &= np.array_equal(adv_totals.cpu().numpy().view(np.uint64), want_adv_totals)
            r["copy_content"] = timed(copy)
            r["nack_fragment_hint_wall"] = walled(lambda: fragment(True))
            r["host_route_wall"] = walled(host_route)
            torch.cuda.synchronize()
            same &= np.array_equal(pin_totals, want_totals)
            used = min(messages, cap) * pitch
            same &= np.array_equal(wire_host_route.cpu().numpy()[:used], want_wire[:used])
            rounds.append(r)
        med = {n: float(np.median([r[n] for r in rounds])) for n in rounds[0]}
        line = dict(workload="ctlmsg", population=name, codec="RS8", k=k, m=m, blocks=nb, segment_size=S, rounds=a.rounds,
                    iters=a.iters, warmup=a.warmup, ms_per_call=[{n: round(v, 4) for n, v in r.items()} for r in rounds],
                    median_ms={n: round(v, 4) for n, v in med.items()},
                    host_route_vs_hinted=[round(r["host_route_wall"] / r["nack_fragment_hint_wall"], 2) for r in rounds],
                    no_hint_vs_host_route=[round(r["nack_fragment_no_hint"] / r["host_route_wall"], 2) for r in rounds],
                    hinted_vs_repair_requests=[round(r["nack_fragment_hint"] / r["repair_requests"], 2) for r in rounds],
                    content_bytes=nbytes, requests=int(want_totals[2]), messages=messages, splits=int(want_totals[3]),
                    wire_bytes=int(want_len[:messages].sum()), adv_limit=int(want_adv_totals[2]),
                    same_as_host_entries=bool(same))
        results.append(line)
        print(json.dumps(line), flush=True)
        del dmask, d_content, d_copy, rows, wire, wire_host_route, ws, pin_content, pin_wire
        torch.cuda.empty_cache()

    if results:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in results:
                f.write(json.dumps(line) + "\n")
        if not all(r["same_as_host_entries"] for r in results):
            raise SystemExit("bench_ctlmsg: the device results differ from the host entries'")
        if not all(x > 1.0 for r in results for x in r["host_route_vs_hinted"]):
            raise SystemExit("bench_ctlmsg: the hinted device call is not faster than the host route")


if __name__ == "__main__":
    main()
