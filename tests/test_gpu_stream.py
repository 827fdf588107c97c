"""Stream objects on the device: nfec_stream_frame, nfec_stream_pack and nfec_stream_unpack.

A NORM stream's sender cuts application writes into segments (NormStreamObject::Write, reference
src/common/normObject.cpp:4039-4232), each behind the 8-byte stream payload header
(include/normMessage.h:1145-1196); its receiver reads the header of every segment to find where the
bytes go (ReadPrivate, :3700-3860).  These tests hold the device frame to the host entry (itself
held to a restatement of the reference loop in tests/test_stream_host.py), pack and unpack to NumPy
loops byte for byte with a -86 fill around everything a call must not write, and the whole chain
writes -> segments -> parity -> wire -> loss -> blocks -> repair -> byte stream returns the stream."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import norm_amd  # noqa: E402
from norm_amd import _native as N  # noqa: E402
from norm_amd import (NFEC_RS8, NFEC_RS16, NFEC_STREAM_EOM as EOM, NFEC_STREAM_FLUSH as FLUSH,  # noqa: E402
                      NormDecoderRS8, NormDecoderRS16, NormEncoderRS8, NormEncoderRS16, StreamState, stream_frame_host)

ENC = {NFEC_RS8: NormEncoderRS8, NFEC_RS16: NormEncoderRS16}
DEC = {NFEC_RS8: NormDecoderRS8, NFEC_RS16: NormDecoderRS16}
FILL = 0xAA  # -86
FILL16 = 0xAAAA
GUARD = 64
BASES = (0, 1, 4, 8, 15)
M32 = 0xFFFFFFFF

# kind, k, m, segment_size, vector, seg_stride, blocks.  1,392 and 1,452 are more than 64 pieces per
# segment; k = 4,096 has several runs per block
SHAPES = [
    (NFEC_RS8, 8, 2, 48, 56, 56, 5),
    (NFEC_RS8, 8, 2, 37, 45, 48, 7),
    (NFEC_RS8, 8, 2, 1, 9, 16, 3),
    (NFEC_RS8, 64, 32, 1392, 1400, 1400, 4),
    (NFEC_RS8, 64, 32, 1452, 1460, 1472, 4),
    (NFEC_RS16, 4096, 256, 56, 64, 64, 2),
]
IDS = ["%d-%d-%d" % (s[1], s[3], s[5]) for s in SHAPES]


@functools.lru_cache(maxsize=None)
def codec(kind, k, m, vec, decoder=False):
    c = (DEC if decoder else ENC)[kind]()
    assert c.Init(k, m, vec)
    return c


def cuda(a, dtype=None):
    a = np.ascontiguousarray(a)
    if dtype is not None:
        a = a.view(dtype)
    return torch.from_numpy(a).cuda()


def dev_bytes(content, base, tail=GUARD):
    """content at `base` bytes past a 64-byte guard in a fresh tensor; (whole tensor, the content's view)"""
    buf = np.full(GUARD + base + len(content) + tail, FILL, np.uint8)
    buf[GUARD + base:GUARD + base + len(content)] = content
    whole = torch.from_numpy(buf).cuda()
    return whole, whole[GUARD + base:GUARD + base + len(content)]


def dev_batch(host):
    """host batch [nb, slots, stride] between two guard blocks of fill"""
    nb = host.shape[0]
    buf = np.full((nb + 2,) + host.shape[1:], FILL, np.uint8)
    buf[1:nb + 1] = host
    whole = torch.from_numpy(buf).cuda()
    return whole, whole[1:nb + 1]


def make_writes(rng, S, want_segments):
    """writes of every kind (empty, 1, S - 1, S, several segments long; every flag pair) that close
    at least want_segments segments; the last one flushes"""
    # (a 1-byte, an S - 1 byte and a full segment, whatever the draws below give)
    lens, flags, est = [1, max(1, S - 1), S, 0], [FLUSH, EOM | FLUSH, 0, FLUSH], 3
    while est < want_segments + 2:
        ln = [0, 1, max(1, S - 1), S, int(rng.integers(0, S + 1)), int(rng.integers(S, 4 * S + 1))][int(rng.integers(0, 6))]
        lens.append(ln)
        flags.append(int(rng.choice([0, 0, EOM, FLUSH, EOM | FLUSH])))
        est += ln // S
    flags[-1] |= FLUSH
    return np.array(lens, np.uint32), np.array(flags, np.uint8)


def header(ln, ms, off):
    return np.frombuffer(int(ln).to_bytes(2, "big") + int(ms).to_bytes(2, "big") + int(off & M32).to_bytes(4, "big"), np.uint8)


# ---- frame ----

def state_of(t):
    return StreamState.from_tensor(t).as_tuple()


@pytest.mark.parametrize("S", [1, 37, 1392])
def test_frame_equals_the_host_rule(S):
    rng = np.random.default_rng(S)
    enc = codec(NFEC_RS8, 8, 2, 1400)
    n = 3 * 1024 + 37  # the scan's tile carry is crossed three times
    kind = rng.integers(0, 8, n)
    lens = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [0, 1, S, max(1, S - 1)],
                     np.where(kind < 6, rng.integers(0, S + 2, n), rng.integers(S, 5 * S + 1, n))).astype(np.uint32)
    flags = rng.choice([0, 0, 0, EOM, FLUSH, EOM | FLUSH], n).astype(np.uint8)
    cases = [(lens, flags, StreamState()),
             (lens, flags, StreamState((1 << 32) - 999, 0, S - 1, (S - 1) // 2, 77)),   # a carry with a message start
             (lens[:1500], flags[:1500] & ~np.uint8(FLUSH), StreamState(5, 1, 0, 0, 3)),  # no cut but position 0
             (lens[:1], flags[:1], StreamState()), (lens[:0], flags[:0], StreamState(9, 0, S // 2, 0, 1))]
    for wl, wf, st0 in cases:
        want_state = st0.copy()
        w_start, w_len, w_ms, w_tot = stream_frame_host(S, wl, wf, want_state)
        total = int(w_tot[0])
        for cap in sorted({total + 5, total, max(total // 2, 1)}):
            dl = cuda(wl, np.int32) if len(wl) else torch.zeros(0, dtype=torch.int32, device="cuda")
            df = cuda(wf) if len(wf) else torch.zeros(0, dtype=torch.uint8, device="cuda")
            g_start, g_len, g_ms, g_tot, g_state = enc.frame_stream(dl, df, st0.copy(), segment_size=S, capacity=cap)
            torch.cuda.synchronize()
            assert g_tot.cpu().numpy().view(np.uint64).tolist() == w_tot.tolist()
            assert state_of(g_state) == want_state.as_tuple()
            for got, want in ((g_start, w_start), (g_len, w_len), (g_ms, w_ms)):
                got = got.cpu().numpy().view(want.dtype)
                head = min(cap, total)
                bad = np.nonzero(got[:head] != want[:head])[0]
                assert bad.size == 0, (S, len(wl), cap, bad[:5], got[bad[:5]], want[bad[:5]])
                assert not got[head:].any()  # nothing past the list's end
        if len(wl) == n:
            assert total > 3 * 1024


# ---- pack ----

def table_for(rng, S, count):
    """a host-framed table of exactly `count` segments and the stream bytes it cuts"""
    lens, flags = make_writes(rng, S, count)
    start, ln, ms, totals = stream_frame_host(S, lens, flags, StreamState())
    assert totals[0] >= count and totals[2] == 0
    data = rng.integers(1, 256, int(lens.sum()), dtype=np.uint8)
    return start[:count].copy(), ln[:count].copy(), ms[:count].copy(), data


def expect_pack(batch, data, table, S, vec, k, first_slot, write_offset, entries, end):
    """(the batch after the call, seg_length rows, num_data, packed, rejected) by a NumPy loop"""
    start, ln, ms = table
    nb = batch.shape[0]
    want = batch.copy()
    lens = np.full((nb, k + 3), FILL16, np.uint16)
    nd = np.full(nb, FILL16, np.uint16)
    ok = rej = 0
    total = entries + (1 if end else 0)
    for i in range(total):
        b, s = divmod(first_slot + i, k)
        if i < entries:
            st, n, m_ = int(start[i]), int(ln[i]), int(ms[i])
            good = 0 < n <= S and st + n <= len(data)
        else:
            st = int(start[entries - 1]) + int(ln[entries - 1]) if entries else 0
            n, m_, good = 0, 0, True
        if b >= nb or not good:
            rej += 1
            continue
        ok += 1
        want[b, s, :8] = header(n, m_, write_offset + st)
        want[b, s, 8:8 + n] = data[st:st + n]
        want[b, s, 8 + n:vec] = 0
        lens[b, s] = 8 + n
    for b in range(nb):
        if first_slot < (b + 1) * k and first_slot + total > b * k:
            nd[b] = min(k, first_slot + total - b * k)
    return want, lens, nd, ok, rej


@pytest.mark.parametrize("kind,k,m,S,vec,stride,nb", SHAPES, ids=IDS)
def test_pack_is_byte_exact(kind, k, m, S, vec, stride, nb):
    rng = np.random.default_rng(k * 7 + S)
    enc = codec(kind, k, m, vec)
    first_slot = k // 2 + 1                      # mid-block
    inside = nb * k - first_slot
    count = inside + 3                           # three entries past the batch's last block
    start, ln, ms, data = table_for(rng, S, count)
    assert {1, max(1, S - 1), S} <= set(ln.tolist())
    # the rejections: too long, empty, past the stream bytes (by one byte)
    bad = rng.choice(inside - 4, 3, replace=False)
    ln[bad[0]] = S + 1
    ln[bad[1]] = 0
    start[bad[2]] = len(data) - int(ln[bad[2]]) + 1
    dtab = (cuda(start, np.int64), cuda(ln, np.int16), cuda(ms, np.int16))
    write_offset = (1 << 32) - int(start[inside // 2])  # the header's offset wraps in mid-batch
    for base in BASES:
        whole_data, ddata = dev_bytes(data, base)
        data_before = whole_data.cpu().numpy()
        # every entry; then a device count two short of the batch's end with the END segment behind it
        for entries, cdev, end in ((count, None, False), (inside - 2, cuda(np.array([inside - 2], np.int64)), True)):
            host = np.full((nb, k + m, stride), FILL, np.uint8)
            whole, dbatch = dev_batch(host)
            nd_all = torch.full((nb + 2,), -21846, dtype=torch.int16, device="cuda")
            lens = torch.full((nb, k + 3), -21846, dtype=torch.int16, device="cuda")
            stats = torch.zeros(2, dtype=torch.int32, device="cuda")
            enc.pack_stream(ddata, *dtab, dbatch, first_slot=first_slot, write_offset=write_offset, count_dev=cdev,
                            end=end, segment_size=S, num_data=nd_all[1:nb + 1], seg_length=lens, stats=stats)
            torch.cuda.synchronize()
            want, w_lens, w_nd, ok, rej = expect_pack(host, data, (start, ln, ms), S, vec, k, first_slot, write_offset,
                                                      entries, end)
            got = whole.cpu().numpy()
            diff = np.argwhere(got[1:nb + 1] != want)
            assert diff.size == 0, (base, end, diff[:4], len(diff))
            assert (got[0] == FILL).all() and (got[nb + 1] == FILL).all()  # the guard blocks
            assert np.array_equal(lens.cpu().numpy().view(np.uint16), w_lens), (base, end)
            got_nd = nd_all.cpu().numpy().view(np.uint16)
            assert np.array_equal(got_nd[1:nb + 1], w_nd) and got_nd[0] == FILL16 and got_nd[-1] == FILL16
            assert stats.cpu().tolist() == [ok, rej] and rej == (6 if not end else 3)
        # without the optional outputs, from slot 0; the stream bytes are only read
        host = np.full((nb, k + m, stride), FILL, np.uint8)
        whole, dbatch = dev_batch(host)
        enc.pack_stream(ddata, *dtab, dbatch, segment_size=S)
        torch.cuda.synchronize()
        want = expect_pack(host, data, (start, ln, ms), S, vec, k, 0, 0, count, False)[0]
        assert np.array_equal(whole.cpu().numpy()[1:nb + 1], want), base
        assert np.array_equal(whole_data.cpu().numpy(), data_before)


# ---- unpack ----

def stream_batch(rng, k, m, S, vec, stride, nb, window_bytes, base_offset):
    """a host batch whose source slots hold stream segments that tile the first bytes of a window
    (in shuffled order), with control segments and headers that claim too much in between;
    returns (batch, per-slot (len, ms, offset), per-slot verdict)"""
    batch = rng.integers(1, 256, (nb, k + m, stride), dtype=np.uint8)
    hdr = np.zeros((nb, k, 3), np.int64)
    verdict = np.zeros((nb, k), np.int64)  # 0 deliver, 2 control, 3 invalid
    slots = [(b, s) for b in range(nb) for s in range(k)]
    order = rng.permutation(len(slots))
    at = 0
    for n, j in enumerate(order):
        b, s = slots[j]
        ln = [1, max(1, S - 1), S, int(rng.integers(1, S + 1))][n % 4]
        off, v = (base_offset + at) & M32, 0
        what = n % 23
        if what == 5:
            ln, v = 0, 2                                  # a control segment (anywhere)
        elif what == 7:
            ln, v = S + 1, 3                              # longer than a segment
        elif what == 9:
            ln, v = 0xFFFF, 3
        elif what == 11:
            off, v = (base_offset - 1) & M32, 3           # one byte before the window: d + len wraps 32 bits
        elif what == 13:
            off, v = (base_offset + window_bytes - ln + 1) & M32, 3   # one byte past its end
        elif what == 15:
            off, v = (base_offset + (1 << 31) + at) & M32, 3   # half the offset space away
        elif what == 17:
            off, v = (base_offset + window_bytes) & M32, 3
        elif at + ln > window_bytes:
            v = 3
        else:
            at += ln
        ms = int(rng.integers(0, max(ln, 1) + 1)) if ln <= S else 7
        hdr[b, s] = (ln, ms, off)
        verdict[b, s] = v
        batch[b, s, :8] = header(ln, ms, off)
    return batch, hdr, verdict


def expect_unpack(batch, hdr, verdict, sel, window_bytes, base_offset):
    win = np.full(window_bytes, FILL, np.uint8)
    nb, k = verdict.shape
    offs = np.full((nb, k + 2), 0xAAAAAAAA, np.uint32)
    lens = np.full((nb, k + 2), FILL16, np.uint16)
    mss = np.full((nb, k + 2), FILL16, np.uint16)
    stats = [0, 0, 0, 0]
    for b in range(nb):
        for s in range(k):
            if not sel[b][s]:
                lens[b, s] = 0xFFFF
                stats[1] += 1
                continue
            ln, ms, off = (int(x) for x in hdr[b, s])
            offs[b, s], lens[b, s], mss[b, s] = off, ln, ms
            stats[int(verdict[b, s])] += 1
            if verdict[b, s] == 0:
                d = (off - base_offset) & M32
                win[d:d + ln] = batch[b, s, 8:8 + ln]
    return win, offs, lens, mss, stats


@pytest.mark.parametrize("kind,k,m,S,vec,stride,nb", SHAPES, ids=IDS)
def test_unpack_is_byte_exact(kind, k, m, S, vec, stride, nb):
    rng = np.random.default_rng(k * 11 + S)
    dec = codec(kind, k, m, vec, True)
    words = (k + m + 31) // 32 + 1
    window_bytes = nb * k * S * 2 // 3 + 5
    base_offset = (1 << 32) - window_bytes // 2          # stream offsets wrap inside the window
    batch, hdr, verdict = stream_batch(rng, k, m, S, vec, stride, nb, window_bytes, base_offset)
    assert {0, 2, 3} <= set(verdict.ravel().tolist())
    dbatch = cuda(batch)
    mask = rng.integers(0, 1 << 32, (nb, words), dtype=np.uint64).astype(np.uint32)
    status = np.where(rng.random(nb) < 0.3, rng.integers(1, m + 1, nb), 0).astype(np.int32)
    status[0], status[1] = 0, 2
    nd = np.full(nb, k, np.uint16)
    nd[nb - 1] = k - 3                                   # the last block was closed early
    by_mask = [[bool((mask[b, s // 32] >> np.uint32(s % 32)) & 1) for s in range(k)] for b in range(nb)]
    every = [[True] * k for _ in range(nb)]
    both = [[bool(status[b] > 0 or by_mask[b][s]) for s in range(k)] for b in range(nb)]
    early = [[s < nd[b] for s in range(k)] for b in range(nb)]
    dmask, dstatus, dnd = cuda(mask, np.int32), cuda(status), cuda(nd, np.int16)
    variants = [(every, None, None, None), (by_mask, dmask, None, None), (both, dmask, dstatus, None),
                ([[bool(status[b] > 0)] * k for b in range(nb)], torch.zeros_like(dmask), dstatus, None),
                (early, None, None, dnd)]
    seen = [0, 0, 0, 0]
    for n, base in enumerate(BASES):
        sel, r, st, num_data = variants[n % len(variants)]
        whole, dwin = dev_bytes(np.full(window_bytes, FILL, np.uint8), base)
        offs = torch.full((nb, k + 2), -1431655766, dtype=torch.int32, device="cuda")  # 0xAAAAAAAA
        lens = torch.full((nb, k + 2), -21846, dtype=torch.int16, device="cuda")
        mss = torch.full((nb, k + 2), -21846, dtype=torch.int16, device="cuda")
        stats = torch.zeros(4, dtype=torch.int32, device="cuda")
        if num_data is None:
            dec.unpack_stream(dbatch, dwin, base_offset=base_offset, received=r, status=st, segment_size=S,
                              offsets=offs, lengths=lens, msg_starts=mss, stats=stats)
        else:  # per-block num_data rides in the batch struct
            b = norm_amd.codec._batch_struct(dbatch, num_data, False)
            N.check(N.lib().nfec_stream_unpack(dec._h, ctypes.byref(b), None, 0, None, dwin.data_ptr(), window_bytes,
                                               base_offset, S, offs.data_ptr(), lens.data_ptr(), mss.data_ptr(), k + 2,
                                               stats.data_ptr(), torch.cuda.current_stream().cuda_stream),
                    "nfec_stream_unpack")
        torch.cuda.synchronize()
        w_win, w_offs, w_lens, w_mss, w_stats = expect_unpack(batch, hdr, verdict, sel, window_bytes, base_offset)
        got = whole.cpu().numpy()
        assert (got[:GUARD + base] == FILL).all() and (got[GUARD + base + window_bytes:] == FILL).all(), base
        diff = np.nonzero(got[GUARD + base:GUARD + base + window_bytes] != w_win)[0]
        assert diff.size == 0, (base, diff[:8], len(diff))
        assert np.array_equal(offs.cpu().numpy().view(np.uint32), w_offs), base
        assert np.array_equal(lens.cpu().numpy().view(np.uint16), w_lens), base
        assert np.array_equal(mss.cpu().numpy().view(np.uint16), w_mss), base
        assert stats.cpu().tolist() == w_stats, (base, w_stats)
        seen = [a + b for a, b in zip(seen, w_stats)]
    assert all(seen), seen  # every verdict was met
    # without the optional outputs; the batch and the mask are only read
    whole, dwin = dev_bytes(np.full(window_bytes, FILL, np.uint8), 3)
    dec.unpack_stream(dbatch, dwin, base_offset=base_offset, received=dmask, segment_size=S)
    torch.cuda.synchronize()
    want = expect_unpack(batch, hdr, verdict, by_mask, window_bytes, base_offset)[0]
    assert np.array_equal(whole.cpu().numpy()[GUARD + 3:GUARD + 3 + window_bytes], want)
    assert np.array_equal(dbatch.cpu().numpy(), batch)
    assert np.array_equal(dmask.cpu().numpy().view(np.uint32), mask)


# ---- arguments ----

def test_argument_errors_launch_nothing():
    k, m, S, vec, stride, nb = 8, 2, 37, 45, 48, 3
    enc = codec(NFEC_RS8, k, m, vec)
    L = N.lib()
    E = N.NFEC_EINVAL
    stream = torch.cuda.current_stream().cuda_stream
    dbatch = torch.full((nb, k + m, stride), FILL, dtype=torch.uint8, device="cuda")
    data = torch.full((400,), FILL, dtype=torch.uint8, device="cuda")
    tab = (torch.zeros(4, dtype=torch.int64, device="cuda"), torch.full((4,), 5, dtype=torch.int16, device="cuda"),
           torch.zeros(4, dtype=torch.int16, device="cuda"))
    lens = torch.full((nb, k), -21846, dtype=torch.int16, device="cuda")
    mask = torch.zeros((nb, 1), dtype=torch.int32, device="cuda")
    stats = torch.zeros(4, dtype=torch.int32, device="cuda")
    b = N.BlockBatch()
    b.blocks, b.block_stride, b.seg_stride, b.nblocks = dbatch.data_ptr(), (k + m) * stride, stride, nb
    seg = N.StreamSegments()
    seg.bytes, seg.stream_bytes, seg.count = data.data_ptr(), 400, 4
    seg.seg_start, seg.seg_len, seg.seg_msg_start = (t.data_ptr() for t in tab)

    def pack(c=enc._h, sg=ctypes.byref(seg), s=S, flags=0, batch=ctypes.byref(b), ls=k, first=0):
        return L.nfec_stream_pack(c, sg, s, first, 0, flags, batch, None, lens.data_ptr(), ls, None, stream)

    def unpack(c=enc._h, batch=ctypes.byref(b), w=data.data_ptr(), s=S, ms=1, os_=k, out=lens.data_ptr()):
        return L.nfec_stream_unpack(c, batch, mask.data_ptr(), ms, None, w, 400, 0, s, None, out, None, os_,
                                    stats.data_ptr(), stream)

    for call in (pack, unpack):
        assert call(c=None) == E and call(batch=None) == E
        assert call(s=0) == E and call(s=vec - 7) == E          # segment_size + 8 <= vector_size
        b.seg_stride = 40                                       # below vector_size
        assert call() == E
        b.seg_stride = stride
    assert pack(sg=None) == E and pack(ls=k - 1) == E and pack(flags=2) == E
    seg.seg_len = None
    assert pack() == E
    seg.seg_len = tab[1].data_ptr()
    seg.bytes = None
    assert pack() == E
    seg.bytes = data.data_ptr()
    assert unpack(w=None) == E and unpack(ms=0) == E and unpack(os_=k - 1) == E
    # the device frame: the host entry's errors, and its own pointers
    wl = torch.full((3,), 5, dtype=torch.int32, device="cuda")
    wf = torch.zeros(3, dtype=torch.uint8, device="cuda")
    totals = torch.zeros(4, dtype=torch.int64, device="cuda")
    sout = torch.zeros(24, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(N.stream_frame_workspace(3, 4) // 8, dtype=torch.int64, device="cuda")

    def frame(c=enc._h, s=S, state=None, so=sout.data_ptr(), t=totals.data_ptr(), w=ws.data_ptr(), o=tab[1].data_ptr()):
        return L.nfec_stream_frame(c, s, wl.data_ptr(), wf.data_ptr(), 3, state or StreamState(), so, tab[0].data_ptr(), o,
                                   tab[2].data_ptr(), 4, t, w, stream)

    assert frame(c=None) == E and frame(s=0) == E and frame(s=65535 - 7) == E and frame(so=None) == E
    assert frame(t=None) == E and frame(w=None) == E and frame(o=None) == E
    assert frame(state=StreamState(carry_bytes=S)) == E
    # nothing to do: NFEC_OK, nothing launched
    b.nblocks = 0
    assert pack() == N.NFEC_OK and unpack() == N.NFEC_OK
    b.nblocks = nb
    seg.count = 0
    assert pack() == N.NFEC_OK
    seg.count = 4
    torch.cuda.synchronize()
    assert (dbatch == FILL).all().item() and (data == FILL).all().item()
    assert (lens == -21846).all().item() and not stats.any().item() and not totals.any().item()
    # and the well-formed calls pass
    assert pack() == N.NFEC_OK and unpack() == N.NFEC_OK and frame() == N.NFEC_OK
    torch.cuda.synchronize()
    assert totals.cpu().tolist() == [0, 0, 15, 1]
    assert stats.cpu().tolist() == [0, nb * k, 0, 0]           # an empty mask selects nothing


# ---- the chain ----

@pytest.mark.parametrize("k,m,S,vec,stride,nb", [(64, 32, 1392, 1400, 1400, 4), (8, 2, 37, 45, 48, 7)])
def test_whole_chain_returns_the_stream(k, m, S, vec, stride, nb):
    """writes -> frame -> pack -> encode -> list / emit -> loss -> ingest -> repair -> unpack, on the device"""
    rng = np.random.default_rng(k * 29 + S)
    enc, dec = codec(NFEC_RS8, k, m, vec), codec(NFEC_RS8, k, m, vec, True)
    nseg = nb * k - 3                              # the last block stays short; END takes one more slot
    lens, flags = make_writes(rng, S, nseg)
    # cut the writes where the host rule has closed just over nseg segments, and flush there
    for n in range(1, len(lens) + 1):
        if int(stream_frame_host(S, lens[:n], flags[:n], StreamState(), 0)[3][0]) >= nseg - 3:
            break
    lens, flags = lens[:n].copy(), flags[:n].copy()
    flags[-1] |= FLUSH
    write_offset = (1 << 32) - int(lens.sum()) // 3   # the stream's offsets wrap on the way
    h_state = StreamState(write_offset=write_offset)
    h_start, h_len, h_ms, h_tot = stream_frame_host(S, lens, flags, h_state)
    total, size = int(h_tot[0]), int(h_tot[1])
    assert nseg - 3 <= total < nb * k and (nb - 1) * k < total and h_tot[2] == 0 and size == lens.sum()
    data = rng.integers(1, 256, size, dtype=np.uint8)
    _, ddata = dev_bytes(data, 5)
    gap, fec_id, fec_m = 13, 5, 8
    # sender: frame, pack (count and state stay on the device), encode, list, emit
    tab = enc.frame_stream(cuda(lens, np.int32), cuda(flags), StreamState(write_offset=write_offset), segment_size=S,
                           capacity=nb * k)
    dev = torch.zeros((nb, k + m, stride), dtype=torch.uint8, device="cuda")
    dnd = torch.zeros(nb, dtype=torch.int16, device="cuda")
    dlens = torch.zeros((nb, k), dtype=torch.int16, device="cuda")
    enc.pack_stream(ddata, tab[0], tab[1], tab[2], dev, write_offset=write_offset, count_dev=tab[3][:1], end=True,
                    segment_size=S, num_data=dnd, seg_length=dlens)
    enc.encode_blocks(dev, num_data=dnd)
    sizes = np.full(nb, k, np.uint16)
    sizes[nb - 1] = total + 1 - (nb - 1) * k
    words = (k + m + 31) // 32
    pend = np.zeros((nb, words), np.uint32)
    for b in range(nb):
        for s in range(int(sizes[b]) + m):
            pend[b, s // 32] |= np.uint32(1 << (s % 32))
    dpend = cuda(pend, np.int32)
    off, blk, sym, ln, start = enc.list_pending(dpend, num_data=dnd, seg_length=dlens, gap=gap)
    count = int(sizes.sum()) + nb * m
    wire = cuda(rng.integers(1, 256, count * (gap + vec) + 40, dtype=np.uint8))
    enc.emit_segments(dev, wire, off, blk, sym, ln, count_dev=start[nb, :1], fec_id=fec_id, fec_m=fec_m, pending=dpend,
                      num_data=dnd)
    torch.cuda.synchronize()
    assert np.array_equal(dnd.cpu().numpy().view(np.uint16), sizes)
    assert state_of(tab[4]) == h_state.as_tuple() and h_state.as_tuple()[2:] == (0, 0, total)
    assert int(start.cpu().numpy().view(np.uint64)[nb, 0]) == count
    # the loss: up to m source segments of every block (the first block none, one block all m)
    h_off, h_blk, h_sym, h_ln = [t.cpu().numpy()[:count] for t in (off, blk, sym, ln)]
    lost = [(b * 5 + 1) % (m + 1) for b in range(nb)]
    lost[0], lost[1] = 0, m
    keep = np.ones(count, bool)
    for b in range(nb):
        src = np.nonzero((h_blk == b) & (h_sym.view(np.uint16) < sizes[b]))[0]
        keep[rng.choice(src, lost[b], replace=False)] = False
    order = rng.permutation(np.nonzero(keep)[0])
    # receiver: intake from the wire, repair, deliver
    dev2 = cuda(rng.integers(1, 256, (nb, k + m, stride), dtype=np.uint8))
    mask = norm_amd.received_mask(nb, k, m)
    dec.ingest_messages(dev2, mask, wire, cuda(h_off[order]), cuda(h_ln[order]), fec_id, fec_m, num_data=dnd)
    st = dec.decode_received(dev2, mask, num_data=dnd)
    whole, dwin = dev_bytes(np.full(size, FILL, np.uint8), 11)
    stats = torch.zeros(4, dtype=torch.int32, device="cuda")
    offs = torch.zeros((nb, k), dtype=torch.int32, device="cuda")
    lens_o = torch.zeros((nb, k), dtype=torch.int16, device="cuda")
    mss = torch.zeros((nb, k), dtype=torch.int16, device="cuda")
    b = norm_amd.codec._batch_struct(dev2, dnd, False)
    N.check(N.lib().nfec_stream_unpack(dec._h, ctypes.byref(b), mask.data_ptr(), mask.shape[1], st.data_ptr(),
                                       dwin.data_ptr(), size, write_offset, S, offs.data_ptr(), lens_o.data_ptr(),
                                       mss.data_ptr(), k, stats.data_ptr(), torch.cuda.current_stream().cuda_stream),
            "nfec_stream_unpack")
    torch.cuda.synchronize()
    assert st.cpu().tolist() == lost
    got = whole.cpu().numpy()
    assert np.array_equal(got[GUARD + 11:GUARD + 11 + size], data)
    assert (got[:GUARD + 11] == FILL).all() and (got[GUARD + 11 + size:] == FILL).all()
    assert stats.cpu().tolist() == [total, nb * k - total - 1, 1, 0]
    # the message starts the receiver rebuilds from the per-slot outputs are the writers': of the
    # writes that start a message, the first in every segment (the header has room for one)
    g_off, g_len, g_ms = (t.cpu().numpy().ravel() for t in (offs, lens_o, mss))
    g_off, g_len, g_ms = g_off.view(np.uint32), g_len.view(np.uint16), g_ms.view(np.uint16)
    live = (g_len != 0xFFFF) & (g_len != 0) & (g_ms != 0)
    rebuilt = sorted(int((int(o) - write_offset + int(s) - 1) & M32) for o, s in zip(g_off[live], g_ms[live]))
    begins, pending, at = [], True, 0
    for wl, wf in zip(lens.tolist(), flags.tolist()):
        if wl and pending:
            begins.append(at)
            pending = False
        at += wl
        pending = pending or bool(wf & EOM)
    ends = (h_start[:total] + h_len[:total]).astype(np.int64)
    seg_of = np.searchsorted(ends, np.array(begins), side="right")
    first_in_segment = [p for i, p in enumerate(begins) if i == 0 or seg_of[i] != seg_of[i - 1]]
    assert rebuilt == first_in_segment and len(rebuilt) > 3
    # the stream end: the control segment's offset is the offset behind the last byte
    ctrl = np.nonzero(g_len == 0)[0]
    assert ctrl.tolist() == [total] and int(g_off[total]) == (write_offset + size) & M32
