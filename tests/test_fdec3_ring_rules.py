"""The LDS column ring of rs8_fdec3's stage 1, walked instruction by instruction as
tools/codegen/gen_fdec_asm.py emits it, for the product's options and for every refill size:

  * a slot is read (ds_read_b64) only after a counted vmcnt wait that retired both DMA pieces of
    the column in it;
  * a slot is re-armed (the DMA that targets it) only after the lgkmcnt(0) that returned the reads
    of the column it held, and only once that column has been read;
  * every vmcnt immediate is the number of pieces issued after the column the next read needs:
    no smaller (the read would race its DMA) and no larger than the pieces in flight;
  * the last vmcnt leaves nothing in flight and the last lgkmcnt(0) no read pending, so that
    stage 2 may park rows in the ring.

The waits are counted in program order, which is how vmcnt and lgkmcnt retire for one wave's
loads of one kind.  Stage 1 has forward branches only (around a column's arithmetic); the walk
checks that no ring instruction lies in a skipped range, so the straight-line order is every
path's order."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "codegen"))
import gen_fdec_asm as g  # noqa: E402

K, NCOL = 64, 80
_M0 = re.compile(r"(?<!\w)m0\b")
OPTIONS = {"product": (), **{f: (f,) for f, o in g.F3_FLAGS.items() if "refill" in o}}


def _walk(lines):
    """-> (columns issued, waits checked); asserts the ring discipline"""
    flight = []                      # DMA pieces in flight, oldest first: (slot, column)
    armed = {}                       # slot -> [column, pieces retired, reads issued, reads returned]
    pending = []                     # ds_reads issued and not yet returned: slots
    m0 = None
    ncols = nwaits = 0
    for n, ln in enumerate(lines):
        op = ln.split()[0]
        if op.startswith("s_cbranch"):
            # the walk goes straight on: the range the branch skips must hold no ring instruction
            end = lines.index(ln.split()[1] + ":", n)
            for x in lines[n + 1:end]:
                assert not (x.split()[0].startswith(("buffer_load", "ds_", "s_waitcnt")) or _M0.search(x)), (n, x)
            continue
        if _M0.search(ln):
            mt = re.fullmatch(r"s_add_u32 m0, %\[wb\], (\d+)", ln)
            assert mt, ln
            m0 = int(mt.group(1))
            assert m0 % g.F3_SLOT == 0 and m0 // g.F3_SLOT < g.F3_NSLOT
        elif op == "buffer_load_dwordx4":
            assert ln.endswith(" lds") and m0 is not None, ln
            slot = m0 // g.F3_SLOT
            second = "offset:1024" in ln
            if not second:
                st = armed.get(slot)
                # re-arm: the column the slot held was read, and its reads have returned
                assert st is None or (st[2] == 4 and st[3] == 4), (n, ln, st)
                assert slot not in pending, (n, ln)
                armed[slot] = [ncols, 0, 0, 0]
                ncols += 1
            else:
                assert flight and flight[-1] == (slot, armed[slot][0]), (n, ln)
            flight.append((slot, armed[slot][0]))
        elif op == "ds_read_b64":
            slot = int(re.search(r"offset:(\d+)", ln).group(1)) // g.F3_SLOT
            st = armed[slot]
            assert st[1] == 2, ("read of a slot whose DMA is in flight", n, ln, st)
            assert st[2] < 4, (n, ln)
            st[2] += 1
            pending.append(slot)
        elif op == "s_waitcnt":
            mt = re.fullmatch(r"s_waitcnt (vmcnt|lgkmcnt)\((\d+)\)", ln)
            assert mt, ln
            imm = int(mt.group(2))
            if mt.group(1) == "lgkmcnt":
                assert imm == 0
                for slot in pending:
                    armed[slot][3] += 1
                pending = []
                continue
            nwaits += 1
            assert imm <= len(flight), ("vmcnt above the pieces in flight", n, ln, len(flight))
            while len(flight) > imm:
                slot, col = flight.pop(0)
                armed[slot][1] += 1
            # the next read's column: every piece of it retired, and the immediate is exactly the
            # pieces issued after it
            nxt = next((x for x in lines[n + 1:] if x.startswith("ds_read_b64")), None)
            if nxt is None:
                assert imm == 0 and not flight
                continue
            slot = int(re.search(r"offset:(\d+)", nxt).group(1)) // g.F3_SLOT
            col = armed[slot][0]
            assert armed[slot][1] == 2, (n, ln)
            assert imm == 2 * (ncols - 1 - col), (n, ln, col, ncols)
            assert all(c > col for _, c in flight)
        else:
            assert not op.startswith(("ds_write", "buffer_store")), ln
    assert not flight and not pending, (flight, pending)
    assert all(st[1:] == [2, 4, 4] for st in armed.values()), armed
    return ncols, nwaits


@pytest.mark.parametrize("name", sorted(OPTIONS))
@pytest.mark.parametrize("m", [32, 16])
def test_ring_discipline(name, m):
    opt = g.f3_opt(OPTIONS[name])
    lines = g.fdec3_stage1(K, m, None, opt)
    ncols, nwaits = _walk(lines)
    assert ncols == NCOL and nwaits == NCOL
    # a refill of R re-arms R slots back to back: the DMA pieces come in runs of 2 R between reads
    runs, cur = [], 0
    for ln in lines:
        if ln.startswith("buffer_load_dwordx4"):
            cur += 1
        elif ln.startswith("ds_read_b64") and cur:
            runs.append(cur)
            cur = 0
    assert runs[0] == 2 * g.F3_NSLOT and set(runs[1:]) == {2 * opt["refill"]}, (name, runs[:4])


def test_load_only_probe_keeps_the_ring():
    """the probe the stream variants are gated on issues the same DMA, waits and ring reads"""
    def ring(lines):
        return [ln for ln in lines if ln.split()[0].startswith(("buffer_load", "ds_read", "s_waitcnt")) or _M0.search(ln)]
    for flags in OPTIONS.values():
        opt = g.f3_opt(flags)
        assert ring(g.fdec3_stage1(K, 32, "nos1", opt)) == ring(g.fdec3_stage1(K, 32, None, opt))


def test_walk_rejects_a_broken_ring():
    """the walk is not vacuous: an early re-arm, a short wait and a late wait all fail it"""
    good = g.fdec3_stage1(K, 32)
    first_rearm = [i for i, ln in enumerate(good) if ln.startswith("s_add_u32 m0")][g.F3_NSLOT]
    lgkm = max(i for i in range(first_rearm) if good[i] == "s_waitcnt lgkmcnt(0)")
    early = good[:lgkm] + good[lgkm + 1:]                      # re-arm before the reads returned
    with pytest.raises(AssertionError):
        _walk(early)
    waits = [i for i, ln in enumerate(good) if ln.startswith("s_waitcnt vmcnt")]
    for delta in (2, -2):
        bad = list(good)
        imm = int(re.search(r"\((\d+)\)", bad[waits[3]]).group(1))
        bad[waits[3]] = f"s_waitcnt vmcnt({imm + delta})"
        with pytest.raises(AssertionError):
            _walk(bad)
