// dispatch_encode.cpp -- encode of a device batch: one ladder of kernels per code (encode_rs8,
// encode_rs16, encode_mdp), the generic kernels below them, and the RS16 Toeplitz pipeline.
// DESIGN.md ("Dispatch") has the ladders as a table.
#include "bitslice.hpp"
#include "codec_state.hpp"

namespace nfec {

// one RS16 product on the tower kernel over a whole vector of t.vec_bytes (even) bytes: its
// 8-byte pieces on the tower kernel, the 2-6 byte tail past them on the tail kernel
// (kernels_gf16tail.hip), so any NORM vector size (segmentSize + 8) stays off the exp-table kernel
bool rs16_tw_full_covers(const Gf16T3Args& t)
{
    const uint32_t even = t.vec_bytes & ~1u, body = even & ~7u;
    if (even == 0) return false;
    Gf16T3Args b = t;
    b.vec_bytes = body;
    return (body == 0 || gf16_tw_covers(b)) && gf16_tw_tail_covers(t, even - body);
}

int launch_rs16_tw_full(const Gf16T3Args& t, hipStream_t s)
{
    const uint32_t even = t.vec_bytes & ~1u, body = even & ~7u;
    if (body) {
        Gf16T3Args b = t;
        b.vec_bytes = body;
        const int rc = launch_gf16_tw_encode(b, s);
        if (rc) return rc;
    }
    return launch_gf16_tw_tail(t, body, even - body, s);
}

}  // namespace nfec

namespace {

// RS16 encode by the Toeplitz split (kernels_tmvp.hip): per sub-batch the prescale of the chunk
// pairs, the three shared-table products in one launch, and the postscale into the parity.
// The sub-batch scratch is the codec's, so calls are ordered: each waits (on its stream) for
// the previous one's end.
// Two Karatsuba levels (tower kernel only): the level-2 prescale writes the pair sums and the
// scaled sums into the block's scratch, launches of the nine (m/4)-row products run into the
// scratch -- each reads, through a column map, the alpha input of its last alpha level (its later
// beta level selects halves) or, with no alpha in its path, the source columns themselves (c
// folded into its coefficients) -- and the level-2 postscale combines them into the m parity rows
// (kernels_tmvp.hip; gf_host.cpp, rs16_tmvp_plan_levels, whose product paths index them).
static int rs16_tmvp2_encode(nfec_codec* c, const nfec_block_batch* b, hipStream_t s)
{
    const int L = c->tmvp_levels;
    const uint32_t k = c->k, m = c->m, r = m >> L, cols = k >> L, vec = c->vec & ~7u;
    uint32_t nprod = 1;
    for (int i = 0; i < L; ++i) nprod *= 3;
    const uint32_t prow0 = k / 2 + 3 * (k / 4);                 // first product row in the scratch
    const uint64_t per_block = (uint64_t)(prow0 + nprod * r) * vec;
    std::lock_guard<std::mutex> lk(c->tmvp_mu);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
        (void)hipGetLastError();
        free_b = 0;
    }
    const uint64_t budget = std::min<uint64_t>(16ull << 30, ((uint64_t)free_b + c->w_tmvp.n) / 2);
    // pipeline: the batch runs as sub-batches whose products launch has about 3,072 workgroups
    // (12 per CU), alternating between the caller's stream and the codec's second one, each
    // stream with its own half of the scratch, each prescale after the previous sub-batch's.  A
    // launch's tail (its last workgroups leave CUs idle) then fills with the other stream's
    // kernels, and the HBM-bound scale kernels run beside the issue-bound products.  Measured
    // (profiles/r06/tmvp_pipe/, one box): RS16(400,100) encode 19.6-19.8 -> 19.1 ms at 16
    // sub-batches (8: 19.2, 32: 19.3, 2-4: no gain), C4 96.3 -> 91.9 ms at 16.
    // NFEC_TMVP_PIPE (knob library): 0 this rule, 1 off, N >= 2 at least N sub-batches
    static const long pipe = diag_knob("NFEC_TMVP_PIPE", 0, 0, 64);
    uint64_t want = 1;
    if (pipe == 0) {
        const uint64_t wg_x4096 = (uint64_t)nprod * (gf16_tw_passes(r, gf16_tw_rows(r)) / 4u) * vec;  // x 4096 per block
        const uint64_t target = std::max<uint64_t>(1, 3072ull * 4096ull / std::max<uint64_t>(wg_x4096, 1));
        want = (b->nblocks + target - 1) / target;
    } else if (pipe >= 2) {
        want = (uint64_t)pipe;
    }
    const bool piped = want >= 2 && b->nblocks >= 2;
    const uint32_t nbuf = piped ? 2u : 1u;
    const uint64_t cap = std::max<uint64_t>(1, budget / nbuf / per_block);
    const uint64_t nsub = std::max<uint64_t>((b->nblocks + cap - 1) / cap, piped ? want : 1u);
    const uint32_t sb = (uint32_t)std::max<uint64_t>(1, (b->nblocks + nsub - 1) / std::max<uint64_t>(nsub, 1));
    if (c->w_tmvp.reserve((size_t)nbuf * sb * per_block) != NFEC_OK) {
        (void)hipGetLastError();
        return NFEC_ENOTSUP;  // no room for the scratch: the one-product encode takes the batch
    }
    if (piped && !c->tmvp_s2) {
        if (hipStreamCreateWithFlags(&c->tmvp_s2, hipStreamNonBlocking) != hipSuccess)
            return hip_fail(hipGetLastError(), "tmvp pipeline stream");
        for (hipEvent_t& ev : c->tmvp_ev)
            NFEC_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    NFEC_HIP(hipStreamWaitEvent(s, c->tmvp_done, 0));
    bool queued = false, forked = false;
    auto leave = [&](int code) {
        // the second stream's work joins the caller's before tmvp_done, so the next encode (any
        // stream) waits for both halves of the scratch
        if (forked && (hipEventRecord(c->tmvp_ev[1], c->tmvp_s2) != hipSuccess ||
                       hipStreamWaitEvent(s, c->tmvp_ev[1], 0) != hipSuccess) && code == NFEC_OK)
            code = hip_fail(hipGetLastError(), "tmvp pipeline join");
        if (queued && hipEventRecord(c->tmvp_done, s) != hipSuccess && code == NFEC_OK)
            code = hip_fail(hipGetLastError(), "tmvp event");
        return code;
    };
    const size_t one_tw = gf16_tw_table_elems(cols, r);
    int rc;
    uint32_t sub = 0;
    for (uint32_t b0 = 0; b0 < b->nblocks; b0 += sb, ++sub) {
        const uint32_t nb = std::min(sb, b->nblocks - b0);
        uint8_t* blocks = static_cast<uint8_t*>(b->blocks) + (uint64_t)b0 * b->block_stride;
        hipStream_t st = s;
        if (piped && (sub & 1u)) {
            if (!forked) {  // the second stream starts after everything before on the caller's
                if (hipEventRecord(c->tmvp_ev[0], s) != hipSuccess ||
                    hipStreamWaitEvent(c->tmvp_s2, c->tmvp_ev[0], 0) != hipSuccess)
                    return leave(hip_fail(hipGetLastError(), "tmvp pipeline fork"));
                forked = true;
            }
            st = c->tmvp_s2;
        }
        // the previous sub-batch's prescale first (the other stream); an error leaves through
        // leave(), so tmvp_done still covers what both streams already hold
        if (piped && sub > 0 && forked && hipStreamWaitEvent(st, c->tmvp_ev[2 + ((sub - 1) & 1u)], 0) != hipSuccess)
            return leave(hip_fail(hipGetLastError(), "tmvp pipeline wait"));
        Rs16TmvpArgs a;
        a.base = blocks;
        a.block_stride = b->block_stride;
        a.seg_stride = b->seg_stride;
        a.nblocks = nb;
        a.vec = vec;
        a.k = k;
        a.cw = m / 2;
        a.hw = r;
        a.sc = c->w_tmvp.p + (piped ? (uint64_t)(sub & 1u) * sb * per_block : 0u);
        a.sc_block_stride = per_block;
        a.cmat = c->d_tmvp_mat.p;
        a.wmat = c->d_tmvp_mat.p + (size_t)k * 16;
        a.gmat = c->d_tmvp_mat.p + (size_t)(k + m) * 16;
        a.num_data = b->num_data ? b->num_data + b0 : nullptr;
        std::vector<Gf16T3Args> e(nprod);
        for (uint32_t pi = 0; pi < nprod; ++pi) {
            int dg[3] = {0, 0, 0};
            for (int l = L, t = (int)pi; l >= 1; --l, t /= 3) dg[l - 1] = t % 3;
            int last_alpha = 0;
            for (int l = 1; l <= L; ++l)
                if (dg[l - 1] == 0) last_alpha = l;
            uint32_t off = 0;  // the beta levels after the last alpha select second halves
            for (int l = last_alpha + 1; l <= L; ++l)
                if (dg[l - 1] == 1) off += m >> l;
            Gf16T3Args& g = e[pi];
            g.nblocks = nb;
            g.k = cols;
            g.m = r;
            g.vec_bytes = vec;
            g.tw = c->d_tmvp_tw.p + pi * one_tw;
            g.out_base = a.sc;
            g.out_block_stride = per_block;
            g.out_seg_stride = vec;
            g.out_slot0 = prow0 + pi * r;
            if (last_alpha == 0) {  // the source columns q m + i + off, chunks of m
                g.base = blocks;
                g.block_stride = b->block_stride;
                g.seg_stride = b->seg_stride;
                g.col_div = r;
                g.col_chunk = m;
                g.col_base = off;
                g.in_slots = k + m;
                // shortened blocks: a source slot at or past the block's numData reads zeros
                g.num_data = a.num_data;
                g.nd_limit = k;
                continue;
            }
            // the alpha input of level last_alpha (block of prefix P' = the digits before it),
            // column q (m >> last_alpha) + i + off
            uint32_t pre = 0;
            for (int l = 1; l < last_alpha; ++l) pre = pre * 3 + (uint32_t)dg[l - 1];
            const uint32_t blk = (last_alpha == 1 ? 0u : k / 2) + pre * (k >> last_alpha);  // level 1: pair sums; 2: s_X
            g.base = a.sc;
            g.block_stride = per_block;
            g.seg_stride = vec;
            g.in_slots = prow0;
            if (last_alpha == L) {
                g.col_base = blk;  // plain columns
            } else {
                g.col_div = r;
                g.col_chunk = m >> last_alpha;
                g.col_base = blk + off;
            }
        }
        // a shape the kernels do not cover shows on the first sub-batch, before any parity byte
        // is written: NFEC_ENOTSUP then hands the batch to the one-product encode
        if ((rc = launch_tmvp2_prescale(a, st)))
            return leave(rc == NFEC_ENOTSUP && b0 == 0 ? rc : fail(rc, "tmvp multi-level prescale"));
        queued = true;
        if (piped && hipEventRecord(c->tmvp_ev[2 + (sub & 1u)], st) != hipSuccess)
            return leave(hip_fail(hipGetLastError(), "tmvp pipeline event"));
        for (uint32_t e0 = 0; e0 < nprod; e0 += kTwMultiMax)
            if ((rc = launch_gf16_tw_multi(e.data() + e0, std::min<uint32_t>(kTwMultiMax, nprod - e0), st)))
                return leave(rc == NFEC_ENOTSUP && b0 == 0 && e0 == 0 ? rc : fail(rc, "tmvp multi-level products"));
        if ((rc = launch_tmvp2_postscale(a, st))) return leave(fail(rc, "tmvp multi-level postscale"));
    }
    return leave(NFEC_OK);
}

static int rs16_tmvp1_encode(nfec_codec* c, const nfec_block_batch* b, hipStream_t s);

// the split over the vector's 8-byte pieces, then (vec % 8 != 0) its last 2-6 bytes on the tail
// kernel with the whole generator: the product is the same at every byte position, so the split
// and the tail write disjoint bytes of the same parity
int rs16_tmvp_encode(nfec_codec* c, const nfec_block_batch* b, hipStream_t s)
{
    const int rc = c->tmvp_levels == 2 ? rs16_tmvp2_encode(c, b, s) : rs16_tmvp1_encode(c, b, s);
    const uint32_t even = c->vec & ~1u, body = even & ~7u;
    if (rc || even == body) return rc;
    Gf16T3Args t;
    t.base = static_cast<const uint8_t*>(b->blocks);
    t.block_stride = b->block_stride;
    t.seg_stride = b->seg_stride;
    t.nblocks = b->nblocks;
    t.k = c->k;
    t.m = c->m;
    t.vec_bytes = even;
    t.tw = c->d_twoff.p;
    t.num_data = b->num_data;
    const int tr = launch_gf16_tw_tail(t, body, even - body, s);
    return tr ? fail(tr, "tmvp vector tail") : NFEC_OK;
}

static int rs16_tmvp1_encode(nfec_codec* c, const nfec_block_batch* b, hipStream_t s)
{
    const uint32_t k = c->k, m = c->m, cw = m / 2, half = k / 2, vec = c->vec & ~7u;
    // sub-batches of at most 16 GiB of scratch (C4's 4,096 blocks: one, 12.5 GB) and at most
    // half of the device memory free now (plus the scratch this codec already holds), of equal
    // size so no launch runs a small tail batch
    const uint64_t per_block = (uint64_t)(half + cw) * vec;
    std::lock_guard<std::mutex> lk(c->tmvp_mu);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
        (void)hipGetLastError();
        free_b = 0;
    }
    const uint64_t budget = std::min<uint64_t>(16ull << 30, ((uint64_t)free_b + c->w_tmvp.n) / 2);
    const uint64_t cap = std::max<uint64_t>(1, budget / per_block);
    const uint64_t nsub = (b->nblocks + cap - 1) / cap;
    const uint32_t sb = (uint32_t)std::max<uint64_t>(1, (b->nblocks + nsub - 1) / std::max<uint64_t>(nsub, 1));
    // no room for the scratch: the one-product shared-table encode (no scratch) takes the batch
    if (c->w_tmvp.reserve((size_t)sb * per_block) != NFEC_OK) {
        (void)hipGetLastError();
        return NFEC_ENOTSUP;
    }
    NFEC_HIP(hipStreamWaitEvent(s, c->tmvp_done, 0));
    // once a kernel that writes the scratch is queued, every exit records tmvp_done after it, so
    // the next Toeplitz encode (any stream) waits for it even when this one hands over
    bool queued = false;
    auto leave = [&](int code) {
        if (queued && hipEventRecord(c->tmvp_done, s) != hipSuccess && code == NFEC_OK)
            code = hip_fail(hipGetLastError(), "tmvp event");
        return code;
    };
    int rc;
    const uint32_t mp = gf16_t3_rows_padded(cw);
    const size_t one = (size_t)(half + 1) * mp * 48;
    const size_t one_tw = gf16_tw_table_elems(half, cw);
    uint32_t shift = 0;
    while ((1u << shift) < cw) ++shift;
    for (uint32_t b0 = 0; b0 < b->nblocks; b0 += sb) {
        const uint32_t nb = std::min(sb, b->nblocks - b0);
        uint8_t* blocks = static_cast<uint8_t*>(b->blocks) + (uint64_t)b0 * b->block_stride;
        Rs16TmvpArgs a;
        a.base = blocks;
        a.block_stride = b->block_stride;
        a.seg_stride = b->seg_stride;
        a.nblocks = nb;
        a.vec = vec;
        a.k = k;
        a.cw = cw;
        a.s = c->w_tmvp.p;
        a.s_block_stride = (uint64_t)half * vec;
        a.x = c->w_tmvp.p + (uint64_t)sb * half * vec;
        a.x_block_stride = (uint64_t)cw * vec;
        a.cmat = c->d_tmvp_mat.p;
        a.wmat = c->d_tmvp_mat.p + (size_t)k * 16;
        a.gmat = c->d_tmvp_mat.p + (size_t)(k + m) * 16;
        a.num_data = b->num_data ? b->num_data + b0 : nullptr;
        Gf16T3Args e[3];
        for (int i = 0; i < 3; ++i) {
            e[i].nblocks = nb;
            e[i].k = half;
            e[i].m = cw;
            e[i].m_pad = mp;
            e[i].vec_bytes = vec;
            if (c->tw) e[i].tw = c->d_tmvp_tw.p + i * one_tw;
            else e[i].offs = c->d_tmvp_off.p + i * one;
            e[i].base = blocks;
            e[i].block_stride = b->block_stride;
            e[i].seg_stride = b->seg_stride;
            e[i].out_base = blocks;
            e[i].out_block_stride = b->block_stride;
            e[i].out_seg_stride = b->seg_stride;
        }
        // P0 = A (pair sums) -> parity rows [k, k + cw)
        e[0].base = a.s;
        e[0].block_stride = a.s_block_stride;
        e[0].seg_stride = vec;
        e[0].out_slot0 = k;
        // P1 over the second column of every pair -> x rows
        e[1].col_shift = shift;
        e[1].col_mask = cw - 1;
        e[1].col_div = c->tw ? cw : 0;  // (any chunk width on the tower kernel)
        e[1].col_chunk = 2 * cw;
        e[1].col_base = cw;
        e[1].in_slots = k + m;
        e[1].out_base = a.x;
        e[1].out_block_stride = a.x_block_stride;
        e[1].out_seg_stride = vec;
        e[1].out_slot0 = 0;
        // P2 over the first column of every pair -> parity rows [k + cw, k + m)
        e[2].col_shift = shift;
        e[2].col_mask = cw - 1;
        e[2].col_div = c->tw ? cw : 0;
        e[2].col_chunk = 2 * cw;
        e[2].col_base = 0;
        e[2].in_slots = k + m;
        e[2].out_slot0 = k + cw;
        if (a.num_data) {
            // shortened blocks (tower kernel only): P1 and P2 mask the source slots at or past
            // the block's numData; P0 (over the pair sums) and P2 write the parity rows after
            // it, slot numData + r
            for (int i = 0; i < 3; ++i) {
                e[i].num_data = a.num_data;
                e[i].nd_limit = k;
            }
            e[0].nd_outputs_only = 1;
            e[0].out_slot0 = 0;
            e[0].out_after_data = 1;
            e[2].out_slot0 = cw;
            e[2].out_after_data = 1;
        }
        // a shape the kernels do not cover shows on the first sub-batch, before any parity byte
        // is written: NFEC_ENOTSUP then hands the batch to the one-product encode
        if ((rc = launch_tmvp_prescale(a, s)))
            return leave(rc == NFEC_ENOTSUP && b0 == 0 ? rc : fail(rc, "tmvp prescale"));
        queued = true;
        if ((rc = c->tw ? launch_gf16_tw_multi(e, 3, s) : launch_gf16_t3_multi(e, 3, s)))
            return leave(rc == NFEC_ENOTSUP && b0 == 0 ? rc : fail(rc, "tmvp products"));
        if ((rc = launch_tmvp_postscale(a, s))) return leave(fail(rc, "tmvp postscale"));
    }
    return leave(NFEC_OK);
}

// the runtime-coefficient kernel's arguments of an RS8 / MDP batch encode (vec_bytes: the whole
// vector; the callers split it into the 8-byte pieces and the tail); false: no table
static bool rt_encode_args(const nfec_codec* c, const nfec_block_batch* b, Rs8RtArgs& a)
{
    if (!c->d_rt.p) return false;
    const bool mdp = c->kind == NFEC_MDP;
    a = Rs8RtArgs();
    a.in_base = static_cast<const uint8_t*>(b->blocks);
    a.in_block_stride = b->block_stride;
    a.in_seg_stride = b->seg_stride;
    a.out_base = static_cast<uint8_t*>(b->blocks);
    a.out_block_stride = b->block_stride;
    a.out_seg_stride = b->seg_stride;
    a.nblocks = b->nblocks;
    a.vec_bytes = c->vec;
    a.k = c->k;
    a.m = c->m;
    a.tab = c->d_rt.p;
    a.tab_col_stride = rs8_rt_col_stride(c->m);
    a.accumulate = (b->flags & NFEC_ACCUMULATE) ? 1u : 0u;
    if (b->num_data) {
        // RS8: flat, each lane's blocks stopping at their own numData (the generator's columns
        // are the same for every numData); MDP: per block, its table depends on numData
        a.per_block = mdp ? 1 : 0;
        a.num_data = b->num_data;
        a.out_after_data = 1;
        if (mdp) {
            a.tab_block_stride = c->rt_block_bytes;
            a.tab_by_count = 1;
        }
    } else {
        a.out_slot0 = c->k;
        if (mdp) a.tab = c->d_rt.p + (uint64_t)(c->k - 1) * (c->rt_block_bytes / 2);
    }
    return true;
}

// the last vec % 8 bytes of an encode whose 8-byte pieces a fast kernel took (kernels_gf8tail.hip)
static int launch_encode_tail(const Rs8RtArgs& a, uint32_t vec, hipStream_t s)
{
    const int rc = launch_rs8_rt_tail(a, vec & ~7u, vec & 7u, s);
    return rc == NFEC_OK ? NFEC_OK : fail(rc == NFEC_ENOTSUP ? NFEC_EDEVICE : rc, "encode tail launch failed");
}

// RS8 / MDP encode on the runtime-coefficient kernel (gen_rs8_rt.hip) over the vector's 8-byte
// pieces, then (vec % 8 != 0, tail set) its last 1-7 bytes on the tail kernel with the same
// arguments; NFEC_ENOTSUP, before anything is launched, for layouts they do not take (offsets
// past 2^31, unaligned batches)
int launch_rt_encode(nfec_codec* c, const nfec_block_batch* b, hipStream_t s, bool& tail)
{
    static const bool use_rt = diag_knob("NFEC_RT", 1) != 0;  // 0: the v_perm kernel (A/B)
    Rs8RtArgs a;
    if (!use_rt || !rt_encode_args(c, b, a)) return NFEC_ENOTSUP;
    const uint32_t vec8 = c->vec & ~7u, nt = c->vec & 7u;
    if (nt && !rs8_rt_tail_covers(a, vec8, nt)) return NFEC_ENOTSUP;
    if (vec8) {
        Rs8RtArgs a8 = a;
        a8.vec_bytes = vec8;
        const int rc = launch_rs8_rt(a8, s);
        if (rc != NFEC_OK) return rc;
    }
    if (!nt) return NFEC_OK;
    tail = true;
    return launch_encode_tail(a, c->vec, s);
}

// ---- one builder per argument struct ----
bs::EncArgs bs_enc_args(const nfec_codec* c, const nfec_block_batch* b)
{
    bs::EncArgs e;
    e.base = static_cast<const uint8_t*>(b->blocks);
    e.out = static_cast<uint8_t*>(b->blocks);
    e.block_stride = b->block_stride;
    e.seg_stride = b->seg_stride;
    e.nblocks = b->nblocks;
    e.vec = c->vec;
    e.num_data = b->num_data;
    e.accumulate = (b->flags & NFEC_ACCUMULATE) ? 1u : 0u;
    e.xcd_remap = bs_flags() & 1u;
    e.nt_store = (bs_flags() >> 1) & 1u;
    return e;
}

// the v_perm kernel over the whole generator; by_count (MDP): the block map of each block's
// numData, one coefficient table per block length
Gf8MatmulArgs gf8_generic_encode_args(const nfec_codec* c, const nfec_block_batch* b, bool by_count)
{
    Gf8MatmulArgs a;
    a.in_base = static_cast<const uint8_t*>(b->blocks);
    a.in_block_stride = b->block_stride;
    a.in_seg_stride = b->seg_stride;
    a.in_count = b->num_data;
    a.cols_const = c->k;
    a.out_base = static_cast<uint8_t*>(b->blocks);
    a.out_block_stride = b->block_stride;
    a.out_seg_stride = b->seg_stride;
    a.out_slot_mode = OUT_SLOT_AFTER_INPUT;
    a.rows_const = c->m;
    a.coef = c->d_coef.p;
    a.coef_col_stride = c->cs;
    if (by_count) {
        a.coef_block_stride = (uint64_t)c->k * c->cs;
        a.coef_by_count = 1;
    }
    a.vtab = c->d_vtab.p;
    a.nblocks = b->nblocks;
    a.vec_bytes = c->vec;
    a.accumulate = (b->flags & NFEC_ACCUMULATE) ? 1u : 0u;
    return a;
}

// the whole generator on the codec's product kernel.  The tower kernel takes shortened batches
// (numData masking per 8-byte piece, parity at slot numData + r) and any even vector size (tail
// kernel); the shared-table kernel unshortened batches with vec % 8 = 0 only
Gf16T3Args gf16_product_args(const nfec_codec* c, const nfec_block_batch* b)
{
    Gf16T3Args t;
    t.base = static_cast<const uint8_t*>(b->blocks);
    t.block_stride = b->block_stride;
    t.seg_stride = b->seg_stride;
    t.nblocks = b->nblocks;
    t.num_data = c->tw ? b->num_data : nullptr;
    t.k = c->k;
    t.m = c->m;
    t.m_pad = gf16_t3_rows_padded(c->m);
    t.vec_bytes = c->vec & ~1u;
    t.offs = c->d_t3off.p;
    t.tw = c->d_twoff.p;
    t.accumulate = (b->flags & NFEC_ACCUMULATE) ? 1u : 0u;
    return t;
}

Gf16BsEncArgs gf16_bs_args(const nfec_codec* c, const nfec_block_batch* b)
{
    Gf16BsEncArgs e;
    e.base = static_cast<const uint8_t*>(b->blocks);
    e.out_base = static_cast<uint8_t*>(b->blocks);
    e.block_stride = b->block_stride;
    e.seg_stride = b->seg_stride;
    e.nblocks = b->nblocks;
    e.num_data = b->num_data;
    e.k = c->k;
    e.m = c->m;
    e.vec_bytes = c->vec & ~1u;
    e.chunks = (e.vec_bytes + 63) / 64;
    e.sel = c->d_sel16.p;
    e.m_pad = gf16_bs_rows_padded(c->m);
    e.accumulate = (b->flags & NFEC_ACCUMULATE) ? 1u : 0u;
    return e;
}

Gf16MatmulArgs gf16_matmul_encode_args(const nfec_codec* c, const nfec_block_batch* b)
{
    Gf16MatmulArgs a;
    a.in_base = static_cast<const uint8_t*>(b->blocks);
    a.in_block_stride = b->block_stride;
    a.in_seg_stride = b->seg_stride;
    a.in_count = b->num_data;
    a.cols_const = c->k;
    a.out_base = static_cast<uint8_t*>(b->blocks);
    a.out_block_stride = b->block_stride;
    a.out_seg_stride = b->seg_stride;
    a.out_slot_mode = OUT_SLOT_AFTER_INPUT;
    a.rows_const = c->m;
    a.coef = reinterpret_cast<const uint16_t*>(c->d_coef.p);
    a.coef_col_stride = c->cs;
    a.exp_tab = reinterpret_cast<const uint16_t*>(c->d_exp.p);
    a.log_tab = c->d_log.p;
    a.nblocks = b->nblocks;
    a.vec_bytes = c->vec & ~1u;
    a.accumulate = (b->flags & NFEC_ACCUMULATE) ? 1u : 0u;
    return a;
}

// ---- the ladders ----
// Each returns NFEC_ENOTSUP, with nothing launched, when none of its kernels takes the batch;
// encode_device_impl then runs the generic kernel.  path is set as each rung is tried, so it names
// the rung that returned.

// A fixed-generator kernel over the vector's 8-byte pieces, then (vec % 8 != 0) the tail kernel
// over the last bytes from the runtime-coefficient table every RS8 / MDP codec has.  NFEC_ENOTSUP
// when the tail kernel does not take this batch (it then keeps the kernels that take whole
// vectors) or the fixed kernel has no body for the shape or layout.
using FixedEncode = int (*)(uint32_t k, uint32_t m, const bs::EncArgs& e, hipStream_t s);

int fixed_then_tail(const nfec_codec* c, const nfec_block_batch* b, bs::EncArgs e, FixedEncode fixed, const char* what,
                    hipStream_t s, int& path, bool& tail)
{
    const uint32_t vec8 = c->vec & ~7u, nt = c->vec & 7u;
    Rs8RtArgs ta;
    if (nt && !(vec8 && rt_encode_args(c, b, ta) && rs8_rt_tail_covers(ta, vec8, nt))) return NFEC_ENOTSUP;
    path = NFEC_PATH_FIXED;
    e.vec = vec8;
    const int rc = fixed(c->k, c->m, e, s);
    if (rc == NFEC_ENOTSUP) return rc;
    if (rc != NFEC_OK) return fail(rc, what);
    if (!nt) return NFEC_OK;
    tail = true;
    return launch_encode_tail(ta, c->vec, s);
}

// (64, 32): the 3-role-wave Karatsuba kernel at 3 waves per SIMD (rs8_enc_t3.hip) for the layouts
// it takes, every other shape and layout the 4-role-wave kernels.  The 2-role-wave kernel
// (rs8_enc_d2.hip) takes exactly t3's batches and is reached only with t3 switched off
// (NFEC_ENC_T3=0 / NFEC_ENC_D2=0, diagnostic library: off; read per call, so one process can run
// all three)
int launch_rs8_d2_or_q4(uint32_t k, uint32_t m, const bs::EncArgs& e, hipStream_t s)
{
    const bool use_t3 = diag_knob("NFEC_ENC_T3", 1) != 0;
    const bool use_d2 = diag_knob("NFEC_ENC_D2", 1) != 0;
    int rc = NFEC_ENOTSUP;
#ifdef NFEC_DIAG
    if (use_t3) rc = launch_rs8_t3_probe(k, m, e, s);  // NFEC_T3_VARIANT: a timing probe
    if (rc == NFEC_ENOTSUP && use_d2) rc = launch_rs8_d2_probe(k, m, e, s);  // NFEC_D2_VARIANT
#endif
    if (rc == NFEC_ENOTSUP && use_t3) rc = launch_rs8_t3_encode(k, m, e, s);
    if (rc == NFEC_ENOTSUP && use_d2) rc = launch_rs8_d2_encode(k, m, e, s);
    if (rc == NFEC_ENOTSUP) rc = launch_rs8_q4_encode(k, m, e, s);
    return rc;
}

int encode_rs8(nfec_codec* c, const nfec_block_batch* b, hipStream_t s, int& path, bool& tail)
{
    if (force_generic()) return NFEC_ENOTSUP;
    // bit-sliced kernels specialised to this (k, m) generator, when they were generated: the
    // hand-allocated assembly kernels first (NFEC_ASM=0 disables them for A/B runs), the 4-role-wave
    // kernels sharing each column's transpose, then the 2-role kernels
    const bs::EncArgs e = bs_enc_args(c, b);
    int rc;
    if (use_asm() && use_q4()) {
        rc = fixed_then_tail(c, b, e, launch_rs8_d2_or_q4, "fixed-generator encode launch failed", s, path, tail);
        if (rc != NFEC_ENOTSUP) return rc;
    }
#ifdef NFEC_DIAG
    if (use_asm()) {
        rc = launch_rs8_asm_encode(c->k, c->m, e, s);
        if (rc != NFEC_ENOTSUP) return rc == NFEC_OK ? NFEC_OK : fail(rc, "assembly encode launch failed");
    }
#endif
    path = NFEC_PATH_FIXED;
    rc = launch_rs8_bitsliced_encode(c->k, c->m, e, s);
    if (rc != NFEC_ENOTSUP) return rc == NFEC_OK ? NFEC_OK : fail(rc, "bit-sliced encode launch failed");
    // any other shape, and shortened batches (per-block mode: the block's numData columns,
    // parity at slot numData + r): bit-sliced with runtime coefficients
    path = NFEC_PATH_RUNTIME;
    return launch_rt_encode(c, b, s, tail);
}

int encode_rs16(nfec_codec* c, const nfec_block_batch* b, hipStream_t s, int& path)
{
    static const bool use_bs16 = diag_knob("NFEC_GF16_BS", 1) != 0;
    const bool acc = b->flags & NFEC_ACCUMULATE;
    int rc;
    // (shortened batches: on the tower kernel, whose products mask each block's source slots at
    // its numData; the prescale masks them too and the postscale writes slot numData + r)
    if (c->tmvp && !acc && (!b->num_data || c->tw)) {
        path = NFEC_PATH_RS16_SPLIT;
        rc = rs16_tmvp_encode(c, b, s);
        if (rc != NFEC_ENOTSUP) return rc;
    }
    if (c->tw || (c->d_t3off.p && !b->num_data)) {
        const Gf16T3Args t = gf16_product_args(c, b);
        path = NFEC_PATH_RS16_PRODUCT;
        rc = !c->tw ? launch_rs16_product(c, t, s) : rs16_tw_full_covers(t) ? launch_rs16_tw_full(t, s) : NFEC_ENOTSUP;
        if (rc != NFEC_ENOTSUP) return rc;
    }
    path = NFEC_PATH_GENERIC;
    return use_bs16 && c->d_sel16.p ? launch_gf16_bs_encode(gf16_bs_args(c, b), s) : NFEC_ENOTSUP;
}

int encode_mdp(nfec_codec* c, const nfec_block_batch* b, hipStream_t s, int& path, bool& tail)
{
    if (force_generic()) return NFEC_ENOTSUP;
    if (!b->num_data && use_asm()) {
        // full blocks: the LFSR's block map is a constant matrix, folded into the bit-sliced
        // assembly bodies of the RS8 encode
        const bs::EncArgs e = bs_enc_args(c, b);
        int rc;
        if (use_q4()) {
            rc = fixed_then_tail(c, b, e, launch_mdp_q4_encode, "MDP q4 encode launch failed", s, path, tail);
            if (rc != NFEC_ENOTSUP) return rc;
        }
#ifdef NFEC_DIAG
        rc = launch_mdp_asm_encode(c->k, c->m, e, s);
        if (rc != NFEC_ENOTSUP) return rc == NFEC_OK ? NFEC_OK : fail(rc, "MDP assembly encode launch failed");
#endif
    }
    // other shapes and shortened blocks (the block map of each block length as a table)
    path = NFEC_PATH_RUNTIME;
    return launch_rt_encode(c, b, s, tail);
}

int encode_device_impl(nfec_codec* c, const nfec_block_batch* b, hipStream_t s, int& path, bool& tail)
{
    // MDP: the in-order LFSR is a linear map of the block; the caller's parity buffers are
    // zeroed at block start by contract, so accumulate has no reference meaning.
    if (c->kind == NFEC_MDP && (b->flags & NFEC_ACCUMULATE))
        return fail(NFEC_ENOTSUP, "MDP encode does not accumulate (LFSR restarts from zeroed parity)");
    const int rc = c->kind == NFEC_RS8    ? encode_rs8(c, b, s, path, tail)
                   : c->kind == NFEC_RS16 ? encode_rs16(c, b, s, path)
                                          : encode_mdp(c, b, s, path, tail);
    if (rc != NFEC_ENOTSUP) return rc;
    path = NFEC_PATH_GENERIC;
    switch (c->kind) {
    case NFEC_RS8: return launch_gf8_matmul(gf8_generic_encode_args(c, b, false), true, s);
    case NFEC_RS16: return launch_gf16_matmul(gf16_matmul_encode_args(c, b), s);
    default: return launch_gf8_matmul(gf8_generic_encode_args(c, b, true), false, s);
    }
}

}  // namespace

// counts each batch encode by the path that took it (nfec_codec_encode_paths)
int nfec::encode_device(nfec_codec* c, const nfec_block_batch* b, hipStream_t s)
{
    int path = NFEC_PATH_GENERIC;
    bool tail = false;
    const int rc = encode_device_impl(c, b, s, path, tail);
    if (rc == NFEC_OK) c->enc_paths[path].fetch_add(1, std::memory_order_relaxed);
    if (rc == NFEC_OK && tail) c->tail_batches[0].fetch_add(1, std::memory_order_relaxed);
    return rc;
}
