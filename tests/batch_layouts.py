"""Batch layouts for the device tests: a batch embedded in a larger pool, and the layout bounds the
dispatchers pick their kernels by.

nfec_block_batch admits any base, seg_stride and block_stride that are multiples of 8 with
seg_stride >= vector_size and block_stride >= (k + m) * seg_stride (check_batch,
nfec_api.cpp:49-61).  A test batch made by torch.from_numpy(dense).cuda() shows one point of that
family: base at an allocation start, block_stride == (k + m) * seg_stride, nothing of the caller's
next to it.  This module places a batch anywhere in a 1-D device pool (embed), keeps a host image of
every byte the call could wrongly touch (Image: the slots with their padding, the gap behind each
block, 4 KiB in front of and behind each block, all seeded junk that differs from region to region),
and restates the 2^31 predicates of dispatch_encode.cpp / dispatch_decode.cpp in plain Python, each
with the line it restates, so a test can ask for the last block_stride a rung takes and the first
it refuses.

Plain module, no GPU needed to import it: torch is imported only by the functions that move bytes.
"""
import bisect
from collections import namedtuple

import numpy as np

F = 1 << 31                  # the 32-bit offset bound of every fast kernel
BAND = 4096                  # bytes compared in front of and behind every block
POOL_CAP = 3 << 30           # one pool, at most 3 GiB: a condition for a shared machine
SLOT_BYTES_WHOLE = 64 << 20  # past this many slot bytes only vec + 64 bytes per slot are kept
GAP_WHOLE = 1 << 20          # a gap up to this size is junk-filled and compared whole


def round_up(x, a):
    return (x + a - 1) // a * a


# ---- layout ----
class Layout(namedtuple("Layout", "lead nb slots seg_stride block_stride")):
    """nb blocks of `slots` slots in a pool: block b at byte lead + b * block_stride."""

    def block(self, b):
        return self.lead + b * self.block_stride

    @property
    def span(self):
        return self.slots * self.seg_stride

    @property
    def extent(self):
        """one past the last byte a test of this layout touches (the band behind the last block)"""
        return self.block(self.nb - 1) + self.span + BAND

    def check(self, k, m, vec):
        """check_batch's rules (nfec_api.cpp:55-59), and room for the band in front"""
        assert self.lead % 8 == 0 and self.seg_stride % 8 == 0 and self.block_stride % 8 == 0
        assert self.seg_stride >= vec
        assert self.slots >= k + m and self.block_stride >= (k + m) * self.seg_stride
        assert self.block_stride >= self.span, "the slots in memory overlap the next block"
        assert self.lead >= BAND
        assert self.extent <= POOL_CAP, (self.extent, POOL_CAP)


def embed(pool, lead, nb, slots_in_memory, seg_stride, block_stride):
    """uint8 view [nb, slots, seg_stride] of a 1-D device tensor with strides (block_stride,
    seg_stride, 1): what _batch_struct (norm_amd/codec.py) turns into an nfec_block_batch"""
    import torch

    assert pool.dim() == 1 and pool.dtype == torch.uint8 and pool.is_contiguous()
    assert lead + (nb - 1) * block_stride + slots_in_memory * seg_stride <= pool.numel()
    return torch.as_strided(pool, (nb, slots_in_memory, seg_stride), (block_stride, seg_stride, 1), lead)


def placements(k, m, vec):
    """The three placements every route runs at (lead counted from a 4 KiB boundary of the pool):
    A base 8 mod 16, no padding, blocks 8 bytes apart; B base 8 mod 256, padded slots, three spare
    slots and 40 bytes behind each block; C wider padding, every other block of a pool."""
    n, s = k + m, round_up(vec, 8)
    return {
        "A": dict(lead=BAND + 8, slots=n, seg_stride=s, block_stride=n * s + 8),
        "B": dict(lead=BAND + 264, slots=n + 3, seg_stride=s + 8, block_stride=(n + 3) * (s + 8) + 40),
        "C": dict(lead=BAND, slots=n, seg_stride=s + 24, block_stride=2 * n * (s + 24)),
    }


# ---- host image of everything near the batch ----
class Image:
    """Host copy of the bytes of a Layout that a call might touch: per block the slots (whole, or
    vec + 64 bytes of each where the batch has more than 64 MiB of slot bytes), the gap behind the
    block (whole up to 1 MiB, else its first 4 KiB) and 4 KiB on either side.  Overlapping regions
    are merged, so every pool byte is held once."""

    def __init__(self, lay, vec, pool_bytes=None):
        self.lay, self.vec = lay, vec
        whole = lay.nb * lay.span <= SLOT_BYTES_WHOLE
        self.width = lay.seg_stride if whole else min(lay.seg_stride, vec + 64)
        gap = lay.block_stride - lay.span
        behind = gap + BAND if gap <= GAP_WHOLE else BAND
        ivs = []
        for b in range(lay.nb):
            s = lay.block(b)
            ivs.append((s - BAND, s))
            if whole:
                ivs.append((s, s + lay.span))
            else:
                ivs += [(s + i * lay.seg_stride, s + i * lay.seg_stride + self.width) for i in range(lay.slots)]
            ivs.append((s + lay.span, s + lay.span + behind))
        hi = pool_bytes if pool_bytes is not None else lay.extent
        ivs = sorted((max(a, 0), min(e, hi)) for a, e in ivs)
        merged = []
        for a, e in ivs:
            if merged and a <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], e)
            elif e > a:
                merged.append([a, e])
        self.starts = [a for a, _ in merged]
        self.bufs = [np.zeros(e - a, np.uint8) for a, e in merged]

    def fill_junk(self, seed):
        """random bytes, a generator of its own per region (never a constant: a kernel that reads
        the wrong place must compute something else)"""
        for i, buf in enumerate(self.bufs):
            buf[:] = np.random.default_rng([seed, i, self.starts[i] & 0xFFFFFFFF]).integers(0, 256, buf.size, dtype=np.uint8)
        return self

    def copy(self):
        c = Image.__new__(Image)
        c.lay, c.vec, c.width, c.starts = self.lay, self.vec, self.width, self.starts
        c.bufs = [b.copy() for b in self.bufs]
        return c

    def slot(self, b, s):
        """the first `width` bytes of slot s of block b, a view into the image"""
        off = self.lay.block(b) + s * self.lay.seg_stride
        i = bisect.bisect_right(self.starts, off) - 1
        o = off - self.starts[i]
        assert 0 <= o and o + self.width <= self.bufs[i].size
        return self.bufs[i][o:o + self.width]

    def upload(self, pool):
        import torch

        for a, buf in zip(self.starts, self.bufs):
            pool[a:a + buf.size].copy_(torch.from_numpy(buf))

    def download(self, pool):
        got = self.copy()
        for i, (a, buf) in enumerate(zip(self.starts, self.bufs)):
            got.bufs[i] = pool[a:a + buf.size].cpu().numpy()
        return got


def put(pool, lay, vec, dense, used, seed):
    """Junk everywhere, then bytes [0, vec) of slots [0, used[b]) of dense block b; uploaded.
    Returns the image as it now is in the pool.  (pool None: host image only.)"""
    img = Image(lay, vec, None if pool is None else pool.numel()).fill_junk(seed)
    for b in range(lay.nb):
        for s in range(int(used[b])):
            img.slot(b, s)[:vec] = dense[b, s, :vec]
    if pool is not None:
        img.upload(pool)
    return img


def get(img, nslots):
    """dense [nb, nslots, vec] of an image"""
    out = np.zeros((img.lay.nb, nslots, img.vec), np.uint8)
    for b in range(img.lay.nb):
        for s in range(nslots):
            out[b, s] = img.slot(b, s)[:img.vec]
    return out


def writable(call, rs16, vec, nd, m, slots, erased=(), decodable=True):
    """[slots, vec] mask of the bytes one block's call may change.  Encode: bytes [0, vec) of slots
    [nd, nd + m), for RS16 [0, vec & ~1) (it codes vec / 2 symbols).  Decode: the same bytes of the
    erased source slots of a decodable block, and nothing else.  Padding is never writable."""
    mask = np.zeros((slots, vec), bool)
    cov = vec & ~1 if rs16 else vec
    if call == "enc":
        mask[nd:nd + m, :cov] = True
    elif decodable:
        for s in erased:
            if s < nd:
                mask[s, :cov] = True
    return mask


def check_untouched(before, after, masks):
    """Every byte outside the writable masks (masks[b]: [slots, vec], False past it) is what was
    put there: the rest of every slot stride of every block, the slots past nd + m, the gap up to
    block_stride and the 4 KiB bands."""
    lay, vec = before.lay, before.vec
    want = before.copy()
    for b in range(lay.nb):
        for s in range(masks[b].shape[0]):
            row = masks[b][s]
            if row.any():   # take the call's bytes where it may write
                want.slot(b, s)[:vec][row] = after.slot(b, s)[:vec][row]
    for a, w, g in zip(want.starts, want.bufs, after.bufs):
        bad = np.nonzero(w != g)[0]
        assert bad.size == 0, ("bytes outside the writable mask changed", bad.size,
                               [(int(a + i) - lay.lead) for i in bad[:8]], lay)


# ---- the predicates, restated ----
def offsets_fit(bs, ss):
    """bitslice.hpp:76-78 (bs::offsets_fit), the fixed-shape RS8 / MDP kernels"""
    return 3 * bs + 256 * ss < F


def t3_takes(nb, vec8, bs, ss):
    """rs8_enc_t3.hip:1171-1176, the RS8(64,32) Karatsuba encode (rs8_enc_d2.hip:1221-1225 the same)"""
    pps = (vec8 + 15) // 16
    if vec8 == 0 or vec8 % 8 or nb == 0 or ss < vec8 or bs < 95 * ss + vec8:
        return False
    span = min(nb, 128 // pps + 2)
    return span * bs + 96 * ss + 16 < F


def rs8_rt_covers(vec8, bs, ss, in_slots, out_slots, per_block):
    """gen_rs8_rt.hip:28696-28701: flat nbg = 2048 / vec + 2, per-block nbg = 1 (in and out share
    the batch's layout in every call of the dispatchers)"""
    if vec8 == 0 or vec8 % 8:
        return False
    nbg = 1 if per_block else 2048 // vec8 + 2
    return nbg * bs + in_slots * ss + vec8 < F and nbg * bs + out_slots * ss + vec8 < F


def rt_tail_covers(vec, ss, bs):
    """kernels_gf8tail.hip:199-210, the layout part (base 8-aligned by check_batch)"""
    vec8, nt = vec & ~7, vec & 7
    return nt != 0 and bs % 8 == 0 and ss % 8 == 0 and vec8 + 8 <= ss and vec8 + nt <= ss


def rt_encode_takes(k, m, vec, bs, ss, per_block):
    """launch_rt_encode, dispatch_encode.cpp:400-416 with rt_encode_args :354-387: flat for RS8 and
    for full MDP blocks (slots k in, k + m out, shortened or not), per block for shortened MDP"""
    vec8, nt = vec & ~7, vec & 7
    if nt and not rt_tail_covers(vec, ss, bs):
        return False
    return vec8 == 0 or rs8_rt_covers(vec8, bs, ss, k, k + m, per_block)


def rt_dec(k, m, vec, bs, ss):
    """dispatch_decode.cpp:363-365, the layout part of rt_dec (RS8_RT).  pass_rs8_rt's own check
    (:832, rs8_rt_covers per block with slot_bound k + m over vec & ~7) is never the tighter one."""
    tails_ok = vec % 8 == 0 or (bs % 8 == 0 and ss % 8 == 0 and (vec & ~7) + 8 <= ss)
    ok = tails_ok and bs + (k + m) * ss + vec < F
    assert not ok or vec < 8 or rs8_rt_covers(vec & ~7, bs, ss, k + m, k + m, True)
    return ok


def mdp_rt_layout(k, m, vec, bs, ss):
    """dispatch_decode.cpp:368-373 (MDP_RT): rs8_rt_covers per block over the k + m survivors, the
    8-byte pieces only, and the tail kernel's layout"""
    vec8, nt = vec & ~7, vec & 7
    tails_ok = nt == 0 or (bs % 8 == 0 and ss % 8 == 0 and vec8 + 8 <= ss)
    return tails_ok and (vec8 == 0 or rs8_rt_covers(vec8, bs, ss, k + m, k + m, True))


def tw_prepare(vec8, bs, ss, slots):
    """gen_gf16_tw.hip:29005-29012 for a product that reads and writes the batch in place (input
    slots k + m; parity at slot k + r, or numData + r <= k + r): nbg = 4096 / vec + 2"""
    if vec8 == 0 or vec8 % 8:
        return False
    return (4096 // vec8 + 2) * bs + slots * ss < F


def t3_prepare(vec, bs, ss, slots):
    """gen_gf16_t3.hip:5634-5639, the shared-table product: nbg = 8192 / vec + 2"""
    if vec == 0 or vec % 8:
        return False
    return (8192 // vec + 2) * bs + slots * ss < F


def tw_full_covers(k, m, vec, bs, ss):
    """rs16_tw_full_covers, dispatch_encode.cpp:12-19: the tower kernel over the 8-byte pieces (the
    tail kernel has no layout bound, kernels_gf16tail.hip:133-138)"""
    even = vec & ~1
    return even != 0 and ((even & ~7) == 0 or tw_prepare(even & ~7, bs, ss, k + m))


def tmvp_offsets_fit(k, m, vec8, bs, ss):
    """kernels_tmvp.hip:117-131 (tmvp1 / tmvp2), the batch side: nb = 512 / (vec / 8) + 2 blocks,
    k + 2 cw = k + m slots.  The scratch side, (nb + 1) x the per-block scratch, does not depend
    on the batch's layout.  512 items of 8 bytes are the tower kernel's 4096-byte group, so this is
    tw_prepare's bound: a layout the split refuses, the tower product refuses too."""
    nb = 512 // max(vec8 // 8, 1) + 2
    return nb * bs + (k + m) * ss < F


def rs16_twdec_covers(k, m, vec, bs, ss):
    """dispatch_decode.cpp:27-53 (RS16_TOWER), the layout part: stage 1 is tw_full_covers with the
    parity rows as accumulate source (slots k + m again), stage 2 writes 32-bit row offsets (:52)"""
    return tw_full_covers(k, m, vec, bs, ss) and (k + m) * ss + vec < F


def flip(pred, lo):
    """(the largest multiple of 8 that pred accepts, the smallest it refuses) for a predicate of
    block_stride that holds at lo and fails from some stride on"""
    assert lo % 8 == 0 and pred(lo), "the predicate refuses the smallest legal block_stride"
    hi = F
    assert not pred(hi)
    a, b = lo // 8, hi // 8          # pred(8 a) holds, pred(8 b) fails
    while b - a > 1:
        c = (a + b) // 2
        if pred(8 * c):
            a = c
        else:
            b = c
    return 8 * a, 8 * b


# ---- the routes, restated (product library: every knob at its default) ----
FIXED_RS8 = ((64, 32), (64, 16), (64, 8))   # has_bitsliced / launch_rs8_q4_encode, gen_rs8_q4.hip:175177-175183
FIXED_MDP = ((64, 32), (64, 16))            # launch_mdp_q4_encode, gen_rs8_q4.hip:175185-175190


def encode_rung(kind, k, m, vec, nb, bs, ss, short=False, acc=False, tower=True, split=False, sel16=True):
    """(counter, rung) of dispatch_encode.cpp's ladders for a batch of this layout.
    RS16: tower: the codec runs the tower kernel (not NFEC_OPT_RS16_SHARED_TABLES); split: it holds
    a Toeplitz split; sel16: its selector table is at most 16 MB (nfec_api.cpp:215)."""
    vec8, nt = vec & ~7, vec & 7
    tail_ok = nt == 0 or (vec8 != 0 and rt_tail_covers(vec, ss, bs))
    if kind == "RS8":
        if (k, m) in FIXED_RS8 and tail_ok:                               # fixed_then_tail, :537-551
            if (k, m) == (64, 32) and not short and t3_takes(nb, vec8, bs, ss):
                return "fixed", "rs8_t3"
            if offsets_fit(bs, ss):                                      # gen_rs8_q4.hip:29057 ...
                return "fixed", "rs8_q4_sh" if short else "rs8_q4"
        if (k, m) in FIXED_RS8 and not short and offsets_fit(bs, ss):    # gen_rs8_bitsliced.hip:25200
            return "fixed", "rs8_enc"
        if rt_encode_takes(k, m, vec, bs, ss, False):
            return "runtime", "rs8_rt"
        return "generic", "gf8_matmul"
    if kind == "MDP":
        if not short and (k, m) in FIXED_MDP and tail_ok and offsets_fit(bs, ss):
            return "fixed", "mdp_q4"
        if rt_encode_takes(k, m, vec, bs, ss, short):
            return "runtime", "rs8_rt"
        return "generic", "gf8_matmul"
    assert kind == "RS16"
    if split and not acc and (not short or tower):                       # encode_rs16, :607-611
        fits = tmvp_offsets_fit(k, m, vec8, bs, ss)
        if tower and fits and tw_prepare(vec8, bs, ss, k + m):
            return "rs16_split", "tmvp_tw"
        if not tower and fits and t3_prepare(vec8, bs, ss, k + m):
            return "rs16_split", "tmvp_t3"
    if tower and tw_full_covers(k, m, vec, bs, ss):                      # :612-617
        return "rs16_product", "gf16_tw"
    if not tower and not short and t3_prepare(vec & ~1, bs, ss, k + m):
        return "rs16_product", "gf16_t3"
    return ("generic", "gf16_bs_encode") if sel16 else ("generic", "gf16_matmul")   # :619, :657


def decode_route(kind, k, m, vec, bs, ss, tower=True, short=False, acc=False):
    """(counter, route) of decode_route, dispatch_decode.cpp:307-394.  RS_GENERIC/product: RS16
    whose stage 1 runs on the product kernel (t3dec, :388 and decode_route_stage1 :400-407: the
    kernel's own bound over the batch, the parity rows as accumulate source at the same layout)."""
    if kind == "RS16":
        if tower and min(k, m) <= 256 and rs16_twdec_covers(k, m, vec, bs, ss):
            return "rs16_tower", "RS16_TOWER"
        covers = tw_prepare(vec, bs, ss, k + m) if tower else t3_prepare(vec, bs, ss, k + m)
        if not short and not acc and vec % 8 == 0 and covers:
            return "generic", "RS_GENERIC/product"
        return "generic", "RS_GENERIC"
    if kind == "MDP":
        return ("runtime", "MDP_RT") if mdp_rt_layout(k, m, vec, bs, ss) else ("generic", "MDP_SOLVE")
    if (k, m) in FIXED_RS8 and offsets_fit(bs, ss):                      # :357-358
        return "fixed", "RS8_FIXED"
    if rt_dec(k, m, vec, bs, ss):
        return "runtime", "RS8_RT"
    return "generic", "RS_GENERIC"


# ---- part two: the ladders walked by layout ----
# One case: a batch, the predicate of block_stride whose two sides it runs at, and the (counter,
# rung) expected at the last stride it accepts and at the first it refuses.  `bound` takes (case, bs).
# expect[0] None: the case runs past the bound only.  es / ep: source erasures and lost parity rows per
# block (decode); opts: a key of the GPU test's codec options.
Ladder = namedtuple("Ladder", "id call kind k m vec nb bound expect short acc opts es ep b0")
Ladder.__new__.__defaults__ = (False, False, "", 0, 0, 0)


def _ss(c):
    return round_up(c.vec, 8)


def _b_offsets_fit(c, bs):
    return offsets_fit(bs, _ss(c))


def _b_rt_dec(c, bs):
    return rt_dec(c.k, c.m, c.vec, bs, _ss(c))


def _b_mdp_rt(c, bs):
    return mdp_rt_layout(c.k, c.m, c.vec, bs, _ss(c))


def _b_twdec(c, bs):
    return rs16_twdec_covers(c.k, c.m, c.vec, bs, _ss(c))


def _b_t3(c, bs):
    return t3_takes(c.nb, c.vec & ~7, bs, _ss(c))


def _b_rt_flat(c, bs):
    return rt_encode_takes(c.k, c.m, c.vec, bs, _ss(c), False)


def _b_tw_full(c, bs):
    return tw_full_covers(c.k, c.m, c.vec, bs, _ss(c))


def _b_t3p(c, bs):
    return t3_prepare(c.vec & ~1, bs, _ss(c), c.k + c.m)


def _b_tmvp(c, bs):
    return tmvp_offsets_fit(c.k, c.m, c.vec & ~7, bs, _ss(c))


SHORT_128 = (128, 100, 90, 127)   # test_decode_shortened_many_erasures_generic_plan's numData

LADDERS = [
    # ---- decode ----
    # four blocks span three strides, a second workgroup follows
    Ladder("dec-rs8-64-32-fixed", "dec", "RS8", 64, 32, 1400, 5, _b_offsets_fit,
           (("fixed", "RS8_FIXED"), ("runtime", "RS8_RT")), es=16),
    Ladder("dec-rs8-64-8-fixed", "dec", "RS8", 64, 8, 1400, 5, _b_offsets_fit,     # the 2-wave fused kernel
           (("fixed", "RS8_FIXED"), ("runtime", "RS8_RT")), es=8),
    Ladder("dec-rs8-20-10-rt", "dec", "RS8", 20, 10, 1003, 2, _b_rt_dec,
           (("runtime", "RS8_RT"), ("generic", "RS_GENERIC")), es=7, ep=2),
    Ladder("dec-rs8-64-32-generic-e16", "dec", "RS8", 64, 32, 1400, 2, _b_rt_dec,
           (None, ("generic", "RS_GENERIC")), es=16),
    Ladder("dec-rs8-64-32-generic-e32", "dec", "RS8", 64, 32, 1400, 2, _b_rt_dec,
           (None, ("generic", "RS_GENERIC")), es=24, ep=8),
    # that test's four blocks as two batches of two (b0: the first): past this bound two blocks
    # span 2 GiB, and the pool holds 3
    Ladder("dec-rs8-128-127-generic-big-plan-a", "dec", "RS8", 128, 127, 72, 2, _b_rt_dec,
           (None, ("generic", "RS_GENERIC")), short=True, es=90, ep=20),
    Ladder("dec-rs8-128-127-generic-big-plan-b", "dec", "RS8", 128, 127, 72, 2, _b_rt_dec,
           (None, ("generic", "RS_GENERIC")), short=True, es=90, ep=20, b0=2),
    Ladder("dec-mdp-64-32", "dec", "MDP", 64, 32, 1397, 2, _b_mdp_rt,
           (("runtime", "MDP_RT"), ("generic", "MDP_SOLVE")), es=-1),            # es -1: block 0 12, block 1 20
    # whole 8-byte vectors: mdp_solve_bs takes block 0 (it refuses vec % 8 != 0 above), gf8_matmul block 1
    Ladder("dec-mdp-64-32-v1400-solve-bs", "dec", "MDP", 64, 32, 1400, 2, _b_mdp_rt,
           (None, ("generic", "MDP_SOLVE")), es=-1),
    Ladder("dec-rs16-40-10-tower", "dec", "RS16", 40, 10, 64, 3, _b_twdec,
           (("rs16_tower", "RS16_TOWER"), ("generic", "RS_GENERIC")), es=6, ep=2),
    # the shared-table codec: stage 1 on the product kernel, then every block on the gather stage
    # (test_rs16_decode_layout_past_the_t3_offset_bound's bound; one counter for both)
    Ladder("dec-rs16-40-10-shared-stage1", "dec", "RS16", 40, 10, 64, 3, _b_t3p,
           (("generic", "RS_GENERIC/product"), ("generic", "RS_GENERIC")), opts="shared", es=6),
    # ---- encode ----
    # span = min(nb, 128 / pps + 2) = 66; the counters cannot tell rs8_t3 from rs8_q4: the rung
    # names here are what tests/test_batch_layouts.py pins
    Ladder("enc-rs8-64-32-t3", "enc", "RS8", 64, 32, 24, 66, _b_t3,
           (("fixed", "rs8_t3"), ("fixed", "rs8_q4"))),
    Ladder("enc-rs8-64-16-fixed", "enc", "RS8", 64, 16, 1408, 4, _b_offsets_fit,
           (("fixed", "rs8_q4"), ("runtime", "rs8_rt"))),
    Ladder("enc-rs8-20-10-rt", "enc", "RS8", 20, 10, 8, 3, _b_rt_flat,
           (("runtime", "rs8_rt"), ("generic", "gf8_matmul"))),
    Ladder("enc-rs8-20-10-rt-acc", "enc", "RS8", 20, 10, 8, 3, _b_rt_flat,
           (("runtime", "rs8_rt"), ("generic", "gf8_matmul")), acc=True),
    Ladder("enc-rs8-20-10-rt-short", "enc", "RS8", 20, 10, 8, 3, _b_rt_flat,
           (("runtime", "rs8_rt"), ("generic", "gf8_matmul")), short=True),
    Ladder("enc-mdp-20-10-rt", "enc", "MDP", 20, 10, 8, 3, _b_rt_flat,
           (("runtime", "rs8_rt"), ("generic", "gf8_matmul"))),
    Ladder("enc-rs16-40-10-bs", "enc", "RS16", 40, 10, 64, 3, _b_tw_full,
           (("rs16_product", "gf16_tw"), ("generic", "gf16_bs_encode")), opts="toeplitz_off"),
    Ladder("enc-rs16-700-200-matmul", "enc", "RS16", 700, 200, 64, 2, _b_tw_full,
           (None, ("generic", "gf16_matmul")), opts="toeplitz_off"),
    Ladder("enc-rs16-32-8-shared", "enc", "RS16", 32, 8, 64, 3, _b_t3p,
           (("rs16_product", "gf16_t3"), ("generic", "gf16_bs_encode")), opts="shared"),
    # the split's bound is the tower product's (tmvp_offsets_fit): past it the batch is generic
    Ladder("enc-rs16-128-32-split", "enc", "RS16", 128, 32, 64, 3, _b_tmvp,
           (("rs16_split", "tmvp_tw"), ("generic", "gf16_bs_encode")), opts="toeplitz_on"),
]
LADDER_BY_ID = {c.id: c for c in LADDERS}


def ladder_num_data(c):
    if not c.short:
        return None
    if (c.k, c.m) == (128, 127):
        return np.array(SHORT_128[c.b0:c.b0 + c.nb], np.uint16)
    return np.array([c.k, 1, c.k - 3, 7, c.k // 2][:c.nb] + [c.k] * max(0, c.nb - 5), np.uint16)


def ladder_sel16(c):
    """the codec holds a selector table (nfec_api.cpp:215: k x rows_padded(m) x 128 bytes <= 16 MB;
    rows padded to 8, nfec_internal.hpp:230)"""
    return c.k * round_up(c.m, 8) * 128 <= (16 << 20)


def ladder_rung(c, bs):
    """the restated dispatcher's answer for the case at block_stride bs"""
    ss = _ss(c)
    if c.call == "dec":
        return decode_route(c.kind, c.k, c.m, c.vec, bs, ss, tower=c.opts != "shared", short=c.short, acc=c.acc)
    return encode_rung(c.kind, c.k, c.m, c.vec, c.nb, bs, ss, short=c.short, acc=c.acc, tower=c.opts != "shared",
                       split=c.opts == "toeplitz_on", sel16=ladder_sel16(c))


def ladder_layouts(c):
    """[(side, Layout, expected (counter, rung))]: the last stride the bound accepts (where the
    case runs both sides) and the first it refuses"""
    ss, n = _ss(c), c.k + c.m
    ok, bad = flip(lambda bs: c.bound(c, bs), n * ss)
    out = []
    for side, bs in (("last-accepted", ok), ("first-refused", bad)):
        if c.expect[side == "first-refused"] is not None:
            out.append((side, Layout(BAND + 8, c.nb, n, ss, bs), c.expect[side == "first-refused"]))
    return out


def pool_bytes():
    """the one pool of part two: the largest extent any case needs, at most 3 GiB"""
    need = max(lay.extent for c in LADDERS for _, lay, _ in ladder_layouts(c))
    assert need <= POOL_CAP, need
    return need
