// dispatch_decode.cpp -- repair of a device batch.  decode_route picks one of six routes from the
// codec and the batch's layout (the only place that reads knobs and layout predicates);
// decode_device_impl sizes the passes, reserves the workspace and runs one pass_* function per
// pass.  DESIGN.md ("Dispatch") has the routes as a table.
#include "bitslice.hpp"
#include "codec_state.hpp"

namespace {

// ---- RS16 decode on the tower kernel, every block ----
// The reference replaces each erased source row of its decoding matrix by the generator row of
// the next surviving parity (normEncoderRS16.cpp:658-716; shortened blocks :675-693) and applies
// the inverse's erased rows (:726-753).  Here, per block, with P_t the substitute parity rows
// and P_last the last of them:
//   stage 1 (flat, the encode itself): z_r = parity row r ^ sum_{c < nd} G[r][c] d_c for every
//           r <= P_last of any block (rows_lim = the batch's largest P_last + 1), with the erased
//           source read as zero (the plan zeroes it) -- so z_{P_t} = sum_s G[P_t][E_s] d_{E_s};
//           shortened blocks mask their columns at numData per 8-byte piece and read their
//           parity at slot numData + r;
//   stage 2 (per block): d_E = A^-1 z over the block's z rows 0..P_last, the inverse laid out by
//           parity row (columns of lost parity rows are zero), written over the erased source.
// With NFEC_ACCUMULATE the erased source is not zeroed: stage 1 then reads its contents X and
// z = A (d_E ^ X), so stage 2's A^-1 z = d_E ^ X written over X is the reference's XOR.  Lost
// parity (uniform loss), shortened blocks, accumulate and any even vector size (the tail kernel)
// all run here; the round-2 exp-table kernel is left for layouts past the tower kernel's 2^31
// offsets and codecs on the shared-table kernel.
static bool rs16_twdec_covers(const nfec_codec* c, const nfec_block_batch* b)
{
    static const bool on = diag_knob("NFEC_RS16_TWDEC", 1) != 0;
    if (!on || c->kind != NFEC_RS16 || !c->tw || !c->d_lwp.p || std::min(c->k, c->m) > kPlanCfMaxE) return false;
    const uint32_t zstride = round_up(c->vec, 8);
    Gf16T3Args t1;  // stage 1's layout (one block: the bounds do not depend on the count)
    t1.base = static_cast<const uint8_t*>(b->blocks);
    t1.block_stride = b->block_stride;
    t1.seg_stride = b->seg_stride;
    t1.nblocks = 1;
    t1.num_data = b->num_data;
    t1.k = c->k;
    t1.m = c->m;
    t1.vec_bytes = c->vec & ~1u;
    t1.tw = c->d_twoff.p;
    t1.accumulate = 1;
    t1.out_base = reinterpret_cast<uint8_t*>(16);  // (any non-null: the z rows' layout)
    t1.out_block_stride = (uint64_t)c->m * zstride;
    t1.out_seg_stride = zstride;
    t1.acc_base = t1.base;
    t1.acc_block_stride = b->block_stride;
    t1.acc_seg_stride = b->seg_stride;
    t1.acc_slot0 = b->num_data ? 0u : c->k;
    t1.acc_after_data = b->num_data ? 1u : 0u;
    // stage 2 writes 32-bit row offsets (erased slot * seg_stride)
    return rs16_tw_full_covers(t1) && (uint64_t)(c->k + c->m) * b->seg_stride + c->vec < (1ull << 31);
}

static int decode_rs16_tw(nfec_codec* c, const nfec_block_batch* b, const uint16_t* locs, uint32_t lstride,
                          const uint16_t* counts, int32_t* status, hipStream_t s)
{
    const bool acc = b->flags & NFEC_ACCUMULATE;
    const uint32_t zstride = round_up(c->vec, 8);
    const uint32_t M2 = std::min(c->k, c->m);              // erased source rows at most
    const uint32_t dcs = round_up(std::max(1u, M2), kRowPad);
    const uint64_t zblk = (uint64_t)c->m * zstride;        // z rows 0..m-1
    const uint64_t c2blk = (uint64_t)c->m * dcs;           // inverse by parity row: [m][dcs]
    const size_t tw2_elems = gf16_tw_table_elems(c->m, M2);  // stage-2 table: m columns, M2 rows
    const uint64_t per_block = zblk + 2ull * c2blk + 2ull * tw2_elems + 4ull * (M2 + 12) + 2ull * c->k + 64;
    uint32_t cap = std::min(b->nblocks, sub_batch(per_block, 8ull << 30, 65536u));
    const uint64_t held = c->ws.z.n + c->ws.coef2.n + 2ull * c->ws.tw2.n;
    if ((uint64_t)cap * per_block > held) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            cap = std::min(cap, sub_batch(per_block, ((uint64_t)free_b + held) / 2, 65536u));
        else
            (void)hipGetLastError();
    }
    const uint32_t npass = (b->nblocks + cap - 1) / std::max(cap, 1u);
    const uint32_t sb = std::max(1u, (b->nblocks + npass - 1) / std::max(npass, 1u));
    int rc;
    if ((rc = c->ws.rows.reserve(sb))) return rc;
    if ((rc = c->ws.rows1.reserve(sb))) return rc;
    if ((rc = c->ws.cols.reserve(sb))) return rc;
    if ((rc = c->ws.rmax.reserve(1))) return rc;
    if (!status && (rc = c->ws.status.reserve(sb))) return rc;
    if ((rc = c->ws.oslots.reserve((size_t)sb * c->k + 128))) return rc;
    if ((rc = c->ws.z.reserve((size_t)sb * zblk))) return rc;
    if ((rc = c->ws.coef2.reserve((size_t)sb * c2blk * 2))) return rc;
    if ((rc = c->ws.tw2.reserve((size_t)sb * tw2_elems))) return rc;
    if ((rc = c->ws.rowoff.reserve((size_t)sb * (M2 + 12)))) return rc;
    uint16_t phi[16];
    uint32_t lam = 0;
    gf16_tw_field(phi, &lam);
    for (uint32_t b0 = 0; b0 < b->nblocks; b0 += sb) {
        const uint32_t nb = std::min(sb, b->nblocks - b0);
        uint8_t* blocks = static_cast<uint8_t*>(b->blocks) + (uint64_t)b0 * b->block_stride;
        const uint16_t* nd = b->num_data ? b->num_data + b0 : nullptr;
        int32_t* st = status ? status + b0 : c->ws.status.p;
        NFEC_HIP(hipMemsetAsync(c->ws.rmax.p, 0, sizeof(uint32_t), s));
        RsPlanArgs p;
        p.bits = 16;
        p.k = c->k;
        p.m = c->m;
        p.nblocks = nb;
        p.num_data = nd;
        p.erasure_locs = locs + (uint64_t)b0 * lstride;
        p.erasure_stride = lstride;
        p.erasure_counts = counts + b0;
        p.gen_parity = c->d_gen.p;
        p.exp_tab = c->d_exp.p;
        p.log_tab = c->d_log.p;
        p.status = st;
        p.rows = c->ws.rows.p;
        p.out_slots2 = c->ws.oslots.p;
        p.cols2 = c->ws.cols.p;
        p.coef_stride = dcs;
        p.coef2 = c->ws.coef2.p;
        p.coef2_block = c2blk;
        p.lwp = c->d_lwp.p;
        p.lw = c->d_lw.p;
        p.by_row = 1;
        p.rows1 = c->ws.rows1.p;
        p.rmax = c->ws.rmax.p;
        p.zero_base = acc ? nullptr : blocks;
        p.zero_block_stride = b->block_stride;
        p.zero_seg_stride = b->seg_stride;
        p.zero_vec = c->vec & ~1u;
        if ((rc = launch_rs_plan(p, s))) return rc;
        // stage 1: z rows 0..rows_lim-1 of every block by the encode, XORed with its parity rows
        Gf16T3Args t;
        t.base = blocks;
        t.block_stride = b->block_stride;
        t.seg_stride = b->seg_stride;
        t.nblocks = nb;
        t.num_data = nd;
        t.k = c->k;
        t.m = c->m;
        t.vec_bytes = c->vec & ~1u;
        t.tw = c->d_twoff.p;
        t.accumulate = 1;
        t.out_base = c->ws.z.p;
        t.out_block_stride = zblk;
        t.out_seg_stride = zstride;
        t.out_slot0 = 0;
        t.acc_base = blocks;
        t.acc_block_stride = b->block_stride;
        t.acc_seg_stride = b->seg_stride;
        t.acc_slot0 = nd ? 0u : c->k;
        t.acc_after_data = nd ? 1u : 0u;
        t.rows_lim = c->ws.rmax.p;
        if ((rc = launch_rs16_tw_full(t, s))) return rc == NFEC_ENOTSUP ? fail(NFEC_EDEVICE, "tower decode stage 1") : rc;
        // stage 2: the per-block tables of A^-1 by parity row, then d_E = A^-1 z
        TwDecTablesArgs d;
        d.coef2 = reinterpret_cast<const uint16_t*>(c->ws.coef2.p);
        d.dcs = dcs;
        d.coef2_block = c2blk;
        d.rows = c->ws.rows.p;
        d.cols = c->ws.cols.p;
        d.out_slots = c->ws.oslots.p;
        d.slots_stride = c->k;
        d.seg_stride = b->seg_stride;
        d.nblocks = nb;
        d.M = M2;
        d.tw = c->ws.tw2.p;
        d.tw_block_stride = tw2_elems;
        d.row_off = c->ws.rowoff.p;
        std::copy(phi, phi + 16, d.phi);
        d.lam = lam;
        if ((rc = launch_tw_dec_tables(d, s))) return rc;
        Gf16T3Args t2;
        t2.base = c->ws.z.p;
        t2.block_stride = zblk;
        t2.seg_stride = zstride;
        t2.nblocks = nb;
        t2.k = c->m;   // columns: z rows 0..P_last (blk_cols)
        t2.m = M2;     // rows: the block's e erased source (blk_rows)
        t2.vec_bytes = c->vec & ~1u;
        t2.tw = c->ws.tw2.p;
        t2.tw_block_stride = tw2_elems;
        t2.blk_rows = c->ws.rows.p;
        t2.blk_cols = c->ws.cols.p;
        t2.row_off = c->ws.rowoff.p;
        t2.row_off_stride = M2 + 12;
        t2.out_base = blocks;
        t2.out_block_stride = b->block_stride;
        t2.out_seg_stride = b->seg_stride;
        if ((rc = launch_rs16_tw_full(t2, s))) return rc == NFEC_ENOTSUP ? fail(NFEC_EDEVICE, "tower decode stage 2") : rc;
    }
    return NFEC_OK;
}

// ---- route ----
enum class Route { RS16_TOWER, MDP_RT, MDP_SOLVE, RS8_FIXED, RS8_RT, RS_GENERIC };

struct DecodeRoute {
    Route kind = Route::RS_GENERIC;
    int dpath = NFEC_DPATH_GENERIC;  // the counter a batch on this route counts in
    uint32_t n = 0;        // slots per block, k + m
    uint32_t E = 0;        // source erasures solved per block at most, min(k, m)
    // RS decode rows: at most E source erasures are solved per block, so the plan's matrices and
    // the z rows are sized by that, not by m (m >> k codes, e.g. npc's auto mode)
    uint32_t dcs = 0, zstride = 0;
    // RS8 / MDP vectors of any length: the bit-sliced repair kernels over the 8-byte pieces (vec8
    // bytes), the tail kernels (kernels_gf8tail.hip) over the last nt bytes.  They read a column's
    // tail as 8 aligned bytes inside its slot (tail_layout; nfec.h asks for this layout anyway); a
    // batch without it keeps the kernels that take whole vectors
    uint32_t vec8 = 0, nt = 0;
    bool tail_layout = false;
    bool big_plan = false;  // min(k, m) > 64: the plan's Gauss-Jordan works in w.work
    // RS16, RS_GENERIC: stage 1 by the product kernel for the blocks whose substitute parities are
    // rows 0..e-1 (t3dec), stage 2 on the tower kernel in per-block mode (tw2); the closed-form
    // inverse when every block's e fits it (cf16)
    bool t3dec = false, tw2 = false, cf16 = false;
    uint32_t np = 0;        // passes of the runtime-coefficient repair's pass-major table (RS8_RT, MDP_RT)
    uint64_t ws_per_block = 0;
    uint32_t max_pass = 65536;
    // knobs of the passes (diagnostic library; read once per process)
    bool fused = true, fdec3 = true, solve = true, solve_bs = true, mdp_bs = true;
    uint32_t lane_major = 2;
};

// one pass of a batch: blocks [b0, b0 + nb) and their lists
struct Pass {
    uint8_t* blocks;
    uint32_t nb;
    const uint16_t *nd, *locs, *counts;
    uint32_t lstride;
    int32_t* status;
};

bool accumulates(const nfec_block_batch* b) { return (b->flags & NFEC_ACCUMULATE) != 0; }

// ---- views: each argument struct is filled in one place per role ----
// the stage-1 rows z of a pass: [block][dcs rows][zstride bytes]
struct ZView {
    uint8_t* base;
    uint64_t block_stride;
    uint32_t seg_stride;
};

ZView z_view(nfec_codec* c, const DecodeRoute& r) { return {c->ws.z.p, (uint64_t)r.dcs * r.zstride, r.zstride}; }

// The repair on the runtime-coefficient kernel, from the pass-major snippet table the plan wrote
// into w.coef1.  RS8: d_E (erased source slots) = W x the block's numData received columns (the
// surviving source and, for an erased one, its substitute parity).  MDP: the plan's matrix over
// the block's survivors, up to k + m columns with a count per block.
Rs8RtArgs rt_repair_args(nfec_codec* c, const nfec_block_batch* b, const DecodeRoute& r, const Pass& p)
{
    const bool mdp = c->kind == NFEC_MDP;
    const uint32_t cols = mdp ? r.n : c->k;
    DecodeWorkspace& w = c->ws;
    Rs8RtArgs a;
    a.in_base = p.blocks;
    a.in_block_stride = b->block_stride;
    a.in_seg_stride = b->seg_stride;
    a.out_base = p.blocks;
    a.out_block_stride = b->block_stride;
    a.out_seg_stride = b->seg_stride;
    a.nblocks = p.nb;
    a.vec_bytes = r.vec8;
    a.k = cols;
    a.m = r.E;
    a.per_block = 1;
    if (mdp) a.blk_cols = w.cols.p;
    else a.num_data = p.nd;
    a.blk_rows = w.rows.p;
    a.in_slots = w.islots.p;
    a.in_slots_stride = cols;
    a.out_slots = w.oslots.p;
    a.out_slots_stride = cols;
    a.tab = reinterpret_cast<const uint16_t*>(w.coef1.p);
    a.tab_block_stride = (uint64_t)r.np * cols * 16;
    a.tab_col_stride = 16;
    a.tab_pass_stride = (uint64_t)cols * 16;
    a.accumulate = accumulates(b);  // (never with MDP)
    a.slot_bound = r.n;
    return a;
}

// RS16 stage 1 by the product kernel for the blocks whose substitute parities are rows 0..e-1
// (RsPlanArgs::rows1): overwrite semantics only, since it zeroes the erased source
// z_t = (encode row t of the block, erased source zeroed) ^ received parity t
Gf16T3Args t3_stage1_args(nfec_codec* c, const nfec_block_batch* b, const DecodeRoute& r, uint8_t* blocks, uint32_t nb)
{
    const ZView z = z_view(c, r);
    Gf16T3Args t;
    t.base = blocks;
    t.block_stride = b->block_stride;
    t.seg_stride = b->seg_stride;
    t.nblocks = nb;
    t.k = c->k;
    t.m = c->m;
    t.m_pad = gf16_t3_rows_padded(c->m);
    t.vec_bytes = c->vec & ~1u;
    t.offs = c->d_t3off.p;
    t.tw = c->d_twoff.p;
    t.accumulate = 1;
    t.out_base = z.base;
    t.out_block_stride = z.block_stride;
    t.out_seg_stride = z.seg_stride;
    t.out_slot0 = 0;
    t.acc_base = blocks;
    t.acc_block_stride = b->block_stride;
    t.acc_seg_stride = b->seg_stride;
    t.acc_slot0 = c->k;
    t.rows_lim = c->ws.rmax.p;
    return t;
}

DecodeRoute decode_route(nfec_codec* c, const nfec_block_batch* b)
{
    // NFEC_RT_DEC=1: the one-pass runtime-coefficient repair for the fixed shapes too, for A/B
    static const bool rt_first = diag_knob("NFEC_RT_DEC", 0) != 0;
    static const bool use_rt = diag_knob("NFEC_RT", 1) != 0;
    // MDP repair on the runtime-coefficient kernel, else the snippet solve / generic kernel
    static const bool use_mdp_rt = diag_knob("NFEC_MDP_RT", 1) != 0;
    // MDP blocks with <= 16 erased source vectors: the snippet solve (NFEC_MDP_BS=0: off)
    static const bool use_mdp_bs = diag_knob("NFEC_MDP_BS", 1) != 0;
    // fused per-block repair for the blocks it qualifies for (NFEC_FUSED=0: off)
    static const bool use_fused = diag_knob("NFEC_FUSED", 1) != 0;
    // 2 (default) = compact lane-major items, idle lanes out of EXEC (1.981-1.985 vs
    // 1.989-1.998 ms, r02g); 0 = item q*64 + lane; 1 = lane L holds items 4L..4L+3
    // (strided loads: 2.16 vs 2.02 ms)
    static const uint32_t lane_major = (uint32_t)diag_knob("NFEC_FDEC_LANEMAJOR", 2, 0, 2);
    // the 3-waves-per-SIMD fused kernel where it applies (NFEC_FDEC3=0: the 2-waves one only)
    static const bool use_fdec3 = diag_knob("NFEC_FDEC3", 1) != 0;
    // NFEC_SOLVE=0: stage 2 on the generic kernel; NFEC_SOLVE_BS=0: no bit-sliced snippet solve
    static const bool use_solve = diag_knob("NFEC_SOLVE", 1) != 0;
    static const bool use_solve_bs = diag_knob("NFEC_SOLVE_BS", 1) != 0;
    // RS16: the closed-form inverse when every block's e fits it (NFEC_RS16_CF=0: Gauss-Jordan)
    static const bool use_cf16 = diag_knob("NFEC_RS16_CF", 1) != 0;

    DecodeRoute r;
    if (rs16_twdec_covers(c, b)) {
        r.kind = Route::RS16_TOWER;
        r.dpath = NFEC_DPATH_RS16_TOWER;
        return r;
    }
    const bool acc = accumulates(b), mdp = c->kind == NFEC_MDP;
    r.n = c->k + c->m;
    r.E = std::min(c->k, c->m);
    r.zstride = round_up(c->vec, 8);
    r.dcs = mdp ? c->cs : round_up(std::max(1u, r.E), kRowPad);
    r.big_plan = !mdp && r.E > 64;
    r.vec8 = c->vec & ~7u;
    r.nt = c->kind == NFEC_RS16 ? 0u : c->vec & 7u;
    r.tail_layout = r.nt && (reinterpret_cast<uintptr_t>(b->blocks) & 7u) == 0 && (b->block_stride & 7u) == 0 &&
                    (b->seg_stride & 7u) == 0 && (uint64_t)r.vec8 + 8u <= b->seg_stride;
    r.np = rs8_rt_passes(r.E);
    r.fused = use_fused;
    r.lane_major = lane_major;
    r.fdec3 = use_fdec3;
    r.solve = use_solve;
    r.solve_bs = use_solve_bs;
    r.mdp_bs = use_mdp_bs;
    const bool tails_ok = !r.nt || r.tail_layout;
    // RS8 shapes with generated fixed-shape kernels (shortened batches too: the plan marks each
    // block's columns past its numData like erased ones, and the repair kernels read its parity at
    // slot numData + t)
    const bool fast = !rt_first && c->kind == NFEC_RS8 && c->m <= 32 && c->k <= 64 && !force_generic() &&
                      has_bitsliced(c->k, c->m) && bs::offsets_fit(b->block_stride, b->seg_stride);
    // RS8 blocks the fused / fixed-shape kernels do not take: a closed-form plan writes each
    // block's whole repair map (e x numData, rs8_plan_rt_kernel) as a pass-major snippet table
    // (8 rows per pass, 16 bytes per column) and ONE pass of the runtime-coefficient kernel
    // computes the erased source from the received columns
    const bool rt_dec = use_rt && !fast && c->kind == NFEC_RS8 && tails_ok && c->d_rt.p && c->d_lwp.p &&
                        !force_generic() &&
                        b->block_stride + (uint64_t)(c->k + c->m) * b->seg_stride + c->vec < (1ull << 31);
    // (the layout is probed before the workspace exists: any non-null table stands in for it, so a
    // codec's first batch takes the same path as its later ones)
    auto mdp_rt_layout = [&]() {
        Rs8RtArgs a = rt_repair_args(c, b, r, Pass{static_cast<uint8_t*>(b->blocks), 1, nullptr, nullptr, nullptr, 0, nullptr});
        if (!a.tab) a.tab = c->d_rt.p;
        return (r.vec8 == 0 || rs8_rt_covers(a)) && (r.nt == 0 || rs8_rt_tail_covers(a, r.vec8, r.nt));
    };
    const bool mdp_rt = mdp && use_mdp_rt && tails_ok && !force_generic() && mdp_rt_layout();
    r.kind = mdp ? (mdp_rt ? Route::MDP_RT : Route::MDP_SOLVE) : fast ? Route::RS8_FIXED : rt_dec ? Route::RS8_RT : Route::RS_GENERIC;
    r.dpath = fast ? NFEC_DPATH_FIXED : (rt_dec || mdp_rt) ? NFEC_DPATH_RUNTIME : NFEC_DPATH_GENERIC;
    // (+ RS16 on the tower kernel: stage 2's per-block snippet tables and row offsets)
    r.ws_per_block = mdp      ? (mdp_rt ? (uint64_t)r.np * r.n * 16 : (uint64_t)r.n * c->cs)
                     : rt_dec ? (uint64_t)r.np * c->k * 16
                              : (uint64_t)r.dcs * r.zstride + ((uint64_t)c->k + r.dcs) * r.dcs * c->sym +
                                    (r.big_plan ? rs_plan_work_bytes(r.dcs, c->sym) : 0) +
                                    (c->tw ? 2ull * gf16_tw_table_elems(r.E, r.E) + 4ull * (r.E + 12) : 0);
    // the runtime-coefficient repair takes passes of up to 1M blocks (its launches stay well
    // below the grid limits): small codes, many blocks, no per-pass launch and plan overhead
    r.max_pass = rt_dec ? (1u << 20) : 65536u;
    if (r.kind != Route::RS_GENERIC || c->kind != NFEC_RS16) return r;
    r.cf16 = use_cf16 && c->d_lwp.p && r.E <= kPlanCfMaxE;
    // the candidates; decode_route_stage1 settles them once the pass size is known
    r.t3dec = (c->d_t3off.p || c->tw) && !b->num_data && !acc && (c->vec % 8) == 0;
    // (NFEC_RS16_TW2 is read per call: the A/B tools flip it inside one process; the per-block
    // row offsets are 32-bit buffer offsets of erased source slots: slot * stride)
    r.tw2 = r.t3dec && c->tw && diag_knob("NFEC_RS16_TW2", 1) != 0 &&
            (uint64_t)c->k * b->seg_stride + c->vec < (1ull << 31);
    return r;
}

// The part of the route that depends on the pass size sb: the plan marks blocks for the
// product-kernel stage 1 only when that kernel takes a pass of the batch's layout (its 2^31 offset
// and grid bounds); otherwise every block keeps the gather stage.  (The z rows may not exist yet:
// any non-null address stands in for them, as they will once reserved.)
void decode_route_stage1(nfec_codec* c, const nfec_block_batch* b, DecodeRoute& r, uint32_t sb)
{
    if (!r.t3dec) return;
    Gf16T3Args t = t3_stage1_args(c, b, r, static_cast<uint8_t*>(b->blocks), sb);
    if (!t.out_base) t.out_base = reinterpret_cast<uint8_t*>(16);
    r.t3dec = c->tw ? gf16_tw_covers(t) : gf16_t3_covers(t);
    r.tw2 = r.tw2 && r.t3dec;
}

// Blocks per pass: passes of equal size, so no launch runs a small tail batch, as large as 8 GiB
// of workspace allows; when that would grow the workspace past what the codec holds, also within
// half of the device memory free now (plus what it holds), so a smaller GPU or several codecs per
// device get smaller passes instead of NFEC_ENOMEM
uint32_t decode_pass_size(const nfec_codec* c, const DecodeRoute& r, uint32_t nblocks)
{
    const DecodeWorkspace& w = c->ws;
    const uint64_t per_block = r.ws_per_block + 4ull * r.n + 64;
    uint32_t cap = std::min(nblocks, sub_batch(per_block, 8ull << 30, r.max_pass));
    const uint64_t held = w.z.n + w.coef1.n + w.coef2.n + w.work.n + 2ull * w.tw2.n;
    if ((uint64_t)cap * per_block > held) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            cap = std::min(cap, sub_batch(per_block, ((uint64_t)free_b + held) / 2, r.max_pass));
        else
            (void)hipGetLastError();
    }
    const uint32_t npass = (nblocks + cap - 1) / std::max(cap, 1u);
    return std::max(1u, (nblocks + npass - 1) / std::max(npass, 1u));
}

// the workspace of a pass of sb blocks on this route
int decode_reserve(nfec_codec* c, const DecodeRoute& r, uint32_t sb, bool have_status)
{
    DecodeWorkspace& w = c->ws;
    const size_t n = r.n, dcs = r.dcs;
    int rc;
    if ((rc = w.rows.reserve(sb))) return rc;
    if ((rc = w.cols.reserve(sb))) return rc;
    if (!have_status && (rc = w.status.reserve(sb))) return rc;
    // + 128: the bit-sliced solves' scalar loads read up to 128 slots past a block's list
    if ((rc = w.islots.reserve(sb * n + 128))) return rc;
    if ((rc = w.oslots.reserve(sb * n + 128))) return rc;
    switch (r.kind) {
    case Route::MDP_RT: return w.coef1.reserve((size_t)sb * r.np * n * 16 + 128);
    case Route::MDP_SOLVE: return w.coef1.reserve(sb * n * dcs);
    case Route::RS8_RT: return w.coef1.reserve((size_t)sb * r.np * c->k * 16 + 128);
    default: break;
    }
    if ((rc = w.coef1.reserve((size_t)sb * c->k * dcs * c->sym))) return rc;
    if ((rc = w.coef2.reserve((size_t)sb * dcs * dcs * c->sym))) return rc;
    if ((rc = w.z.reserve((size_t)sb * dcs * r.zstride))) return rc;
    if (r.big_plan && (rc = w.work.reserve((size_t)sb * rs_plan_work_bytes(r.dcs, c->sym)))) return rc;
    if (r.t3dec) {
        if ((rc = w.rows1.reserve(sb))) return rc;
        if ((rc = w.rmax.reserve(1))) return rc;
    }
    if (r.tw2) {  // tables of E rows per block
        if ((rc = w.tw2.reserve((size_t)sb * gf16_tw_table_elems(r.E, r.E)))) return rc;
        if ((rc = w.rowoff.reserve((size_t)sb * (r.E + 12)))) return rc;
    }
    if (r.kind == Route::RS8_FIXED) {
        if ((rc = w.emask.reserve((size_t)sb * 2))) return rc;
        if ((rc = w.psel.reserve((size_t)sb * 2))) return rc;
        if ((rc = w.pmap.reserve((size_t)sb * c->m))) return rc;
        if ((rc = w.gate.reserve(1))) return rc;
    }
    return NFEC_OK;
}

// ---- MDP ----
MdpPlanArgs mdp_plan_args(nfec_codec* c, const DecodeRoute& r, const Pass& p)
{
    DecodeWorkspace& w = c->ws;
    MdpPlanArgs a;
    a.k = c->k;
    a.m = c->m;
    a.nblocks = p.nb;
    a.num_data = p.nd;
    a.erasure_locs = p.locs;
    a.erasure_stride = p.lstride;
    a.erasure_counts = p.counts;
    a.exp_tab = c->d_exp.p;
    a.log_tab = c->d_log.p;
    a.status = p.status;
    a.rows = w.rows.p;
    a.cols = w.cols.p;
    a.in_slots = w.islots.p;
    a.out_slots = w.oslots.p;
    a.coef_stride = r.dcs;
    a.coef = w.coef1.p;
    if (r.kind == Route::MDP_RT) {  // the matrix as snippet offsets, pass-major
        a.coef16 = reinterpret_cast<uint16_t*>(w.coef1.p);
        a.npass16 = r.np;
    }
    return a;
}

MdpSolveArgs mdp_solve_args(nfec_codec* c, const nfec_block_batch* b, const DecodeRoute& r, const Pass& p)
{
    DecodeWorkspace& w = c->ws;
    MdpSolveArgs a;
    a.base = p.blocks;
    a.block_stride = b->block_stride;
    a.seg_stride = b->seg_stride;
    a.nblocks = p.nb;
    a.vec = c->vec;
    a.rows = w.rows.p;
    a.cols = w.cols.p;
    a.in_slots = w.islots.p;
    a.out_slots = w.oslots.p;
    a.slots_stride = r.n;
    a.coef = w.coef1.p;
    a.coef_block_stride = (uint64_t)r.n * r.dcs;
    a.coef_col_stride = r.dcs;
    return a;
}

// the plan's matrix over the block's survivors on the generic kernel
Gf8MatmulArgs mdp_generic_args(nfec_codec* c, const nfec_block_batch* b, const DecodeRoute& r, const Pass& p)
{
    DecodeWorkspace& w = c->ws;
    Gf8MatmulArgs a;
    a.in_base = p.blocks;
    a.in_block_stride = b->block_stride;
    a.in_seg_stride = b->seg_stride;
    a.in_slots = w.islots.p;
    a.in_count = w.cols.p;
    a.out_base = p.blocks;
    a.out_block_stride = b->block_stride;
    a.out_seg_stride = b->seg_stride;
    a.out_slots = w.oslots.p;
    a.out_slot_mode = OUT_SLOT_LIST;
    a.row_count = w.rows.p;
    a.slots_stride = r.n;
    a.coef = w.coef1.p;
    a.coef_block_stride = (uint64_t)r.n * r.dcs;
    a.coef_col_stride = r.dcs;
    a.vtab = c->d_vtab.p;
    a.nblocks = p.nb;
    a.vec_bytes = c->vec;
    return a;
}

// plan, then MDP_RT: one pass of the runtime-coefficient kernel over the survivors (+ tail);
// MDP_SOLVE: the snippet solve for the blocks it takes, the generic kernel for the rest
int pass_mdp(nfec_codec* c, const nfec_block_batch* b, const DecodeRoute& r, const Pass& p, hipStream_t s, bool& tail)
{
    int rc;
    if ((rc = launch_mdp_plan(mdp_plan_args(c, r, p), s))) return rc;
    if (r.kind == Route::MDP_RT) {
        const Rs8RtArgs a = rt_repair_args(c, b, r, p);
        if (r.vec8 && (rc = launch_rs8_rt(a, s)))
            return fail(rc == NFEC_ENOTSUP ? NFEC_EDEVICE : rc, "MDP runtime-coefficient repair launch failed");
        if (r.nt) {
            if ((rc = launch_rs8_rt_tail(a, r.vec8, r.nt, s)))
                return fail(rc == NFEC_ENOTSUP ? NFEC_EDEVICE : rc, "MDP repair tail launch failed");
            tail = true;
        }
        return NFEC_OK;
    }
    if (r.mdp_bs) {
        rc = launch_mdp_solve_bs(mdp_solve_args(c, b, r, p), s);
        if (rc != NFEC_OK && rc != NFEC_ENOTSUP) return fail(rc, "MDP solve launch failed");
    }
    return launch_gf8_matmul(mdp_generic_args(c, b, r, p), false, s);
}

// ---- RS8 on the fixed-shape kernels ----
RsPlan2Args plan2_args(nfec_codec* c, const DecodeRoute& r, const Pass& p)
{
    DecodeWorkspace& w = c->ws;
    RsPlan2Args a;
    a.k = c->k;
    a.m = c->m;
    a.nblocks = p.nb;
    a.num_data = p.nd;
    a.erasure_locs = p.locs;
    a.erasure_stride = p.lstride;
    a.erasure_counts = p.counts;
    a.exp_tab = c->d_exp.p;
    a.log_tab = c->d_log.p;
    a.lwp = c->d_lwp.p;
    a.lw = c->d_lw.p;
    a.status = p.status;
    a.rows = w.rows.p;
    a.cols2 = w.cols.p;
    a.out_slots2 = w.oslots.p;
    a.emask = w.emask.p;
    a.psel = w.psel.p;
    a.pmap = w.pmap.p;
    a.coef_stride = r.dcs;
    a.coef2 = w.coef2.p;
    return a;
}

// segment tails: every kernel of this route over the 8-byte pieces, the tail kernel (after the
// plan, before the fused kernel clears rows / psel) over the last nt bytes of every decodable block
Rs8FixedDecTailArgs fixed_tail_args(nfec_codec* c, const nfec_block_batch* b, const DecodeRoute& r, const Pass& p)
{
    DecodeWorkspace& w = c->ws;
    Rs8FixedDecTailArgs a;
    a.base = p.blocks;
    a.block_stride = b->block_stride;
    a.seg_stride = b->seg_stride;
    a.nblocks = p.nb;
    a.k = c->k;
    a.m = c->m;
    a.num_data = p.nd;
    a.rows = w.rows.p;
    a.emask = w.emask.p;
    a.psel = w.psel.p;
    a.pmap = w.pmap.p;
    a.out_slots = w.oslots.p;
    a.slots_stride = c->k;
    a.coef2 = w.coef2.p;
    a.coef_stride = r.dcs;
    a.fused_rows = std::min(16u, c->m);
    a.gen = c->d_gen.p;
    a.accumulate = accumulates(b);
    return a;
}

// the fused per-block repair over fvec bytes of every vector
FdecArgs fdec_args(nfec_codec* c, const nfec_block_batch* b, const DecodeRoute& r, const Pass& p, uint32_t fvec)
{
    DecodeWorkspace& w = c->ws;
    FdecArgs a;
    a.base = p.blocks;
    a.block_stride = b->block_stride;
    a.seg_stride = b->seg_stride;
    a.nblocks = p.nb;
    a.vec = fvec;
    a.ips = fvec / 8;
    a.rows = w.rows.p;
    a.psel = w.psel.p;
    a.emask = w.emask.p;
    a.coef = w.coef2.p;
    a.coef_block_stride = (uint64_t)r.dcs * r.dcs;
    a.coef_col_stride = r.dcs;
    a.out_slots = w.oslots.p;
    a.slots_stride = c->k;
    a.accumulate = accumulates(b);
    a.num_data = p.nd;
    a.lane_major = r.lane_major;
    a.xcd_remap = bs_flags() & 1u;
    return a;
}

// stage 1 of the unfused repair: z by the bit-sliced re-encode with the erased columns masked
bs::DecArgs reencode_args(nfec_codec* c, const nfec_block_batch* b, const DecodeRoute& r, const Pass& p, uint32_t fvec,
                          const uint32_t* gate, uint32_t gen)
{
    DecodeWorkspace& w = c->ws;
    const ZView z = z_view(c, r);
    bs::DecArgs a;
    a.base = p.blocks;
    a.block_stride = b->block_stride;
    a.seg_stride = b->seg_stride;
    a.nblocks = p.nb;
    a.vec = fvec;
    a.emask = w.emask.p;
    a.psel = w.psel.p;
    a.pmap = w.pmap.p;
    a.z = z.base;
    a.z_block_stride = z.block_stride;
    a.z_stride = z.seg_stride;
    a.xcd_remap = bs_flags() & 1u;
    a.gate = gate;
    a.gate_gen = gen;
    a.num_data = p.nd;
    return a;
}

// stage 2, d_E = A^-1 z into the erased slots, on the solve kernels
Gf8SolveArgs solve_args(nfec_codec* c, const nfec_block_batch* b, const DecodeRoute& r, const Pass& p, uint32_t fvec,
                        const uint32_t* gate, uint32_t gen)
{
    DecodeWorkspace& w = c->ws;
    const ZView z = z_view(c, r);
    Gf8SolveArgs a;
    a.z = z.base;
    a.z_block_stride = z.block_stride;
    a.z_stride = z.seg_stride;
    a.cols = w.cols.p;
    a.rows = w.rows.p;
    a.out_slots = w.oslots.p;
    a.slots_stride = c->k;
    a.out = p.blocks;
    a.out_block_stride = b->block_stride;
    a.out_seg_stride = b->seg_stride;
    a.coef = w.coef2.p;
    a.coef_block_stride = (uint64_t)r.dcs * r.dcs;
    a.coef_col_stride = r.dcs;
    a.vtab = c->d_vtab.p;
    a.nblocks = p.nb;
    a.vec_bytes = fvec;
    a.accumulate = accumulates(b);
    a.gate = gate;
    a.gate_gen = gen;
    return a;
}

// ... and the same on the generic kernel (NFEC_SOLVE=0 on the fixed route; the generic route)
Gf8MatmulArgs stage2_gf8_args(nfec_codec* c, const nfec_block_batch* b, const DecodeRoute& r, const Pass& p,
                              uint32_t vec_bytes)
{
    DecodeWorkspace& w = c->ws;
    const ZView z = z_view(c, r);
    Gf8MatmulArgs a;
    a.in_base = z.base;
    a.in_block_stride = z.block_stride;
    a.in_seg_stride = z.seg_stride;
    a.in_count = w.cols.p;
    a.out_base = p.blocks;
    a.out_block_stride = b->block_stride;
    a.out_seg_stride = b->seg_stride;
    a.out_slots = w.oslots.p;
    a.out_slot_mode = OUT_SLOT_LIST;
    a.row_count = w.rows.p;
    a.slots_stride = c->k;
    a.coef = w.coef2.p;
    a.coef_block_stride = (uint64_t)r.dcs * r.dcs;
    a.coef_col_stride = r.dcs;
    a.vtab = c->d_vtab.p;
    a.nblocks = p.nb;
    a.vec_bytes = vec_bytes;
    a.accumulate = accumulates(b);
    return a;
}

// Closed-form plan, then in this order: the tail kernel (it reads rows / psel before the fused
// kernel clears them), the fused per-block repair for the blocks it qualifies for, and for the
// blocks it left the bit-sliced re-encode (z) and the e x e solve.  The unfused kernels skip the
// blocks the fused one marked, and their whole launch when the plan left the gate shut.
int pass_rs8_fixed(nfec_codec* c, const nfec_block_batch* b, const DecodeRoute& r, const Pass& p, hipStream_t s, bool& tail)
{
    DecodeWorkspace& w = c->ws;
    int rc;
    RsPlan2Args p2 = plan2_args(c, r, p);
    Rs8FixedDecTailArgs ft = fixed_tail_args(c, b, r, p);
    const bool split = r.tail_layout && rs8_fixed_dec_tail_covers(ft, r.vec8, r.nt);
    const uint32_t fvec = split ? r.vec8 : c->vec;  // what the other kernels take
    const FdecArgs f = fdec_args(c, b, r, p, fvec);
    const bool fused = r.fused && fvec && rs8_fused_decode_covers(c->k, c->m, f);
    // gate: the plan writes this pass's generation into w.gate when some block needs the
    // unfused kernels; when the fused kernel ran they skip their whole launch otherwise
    const uint32_t gen = ++w.gate_gen;
    if (fused) {
        p2.gate = w.gate.p;
        p2.gate_gen = gen;
        p2.fused_rows = std::min(16u, c->m);  // the inverse of the blocks it takes, by row
    }
    if ((rc = launch_rs_plan2(p2, s))) return rc;
    if (split) {
        ft.fused_rows = p2.fused_rows;
        if ((rc = launch_rs8_fixed_dec_tail(ft, r.vec8, r.nt, s)))
            return fail(rc == NFEC_ENOTSUP ? NFEC_EDEVICE : rc, "fixed-shape repair tail launch failed");
        tail = true;
        if (!fvec) return NFEC_OK;  // no 8-byte piece: the tail kernel repaired the whole vector
    }
    const uint32_t* gate = nullptr;
    if (fused) {
        // the 3-waves-per-SIMD kernel where it applies (lane-major items, segments up to
        // 1,664 B, m = 32 or 16), else the 2-waves one
        rc = r.fdec3 ? launch_rs8_fdec3(c->k, c->m, f, s) : NFEC_ENOTSUP;
        if (rc == NFEC_ENOTSUP) rc = launch_rs8_fused_decode(c->k, c->m, f, s);
        if (rc != NFEC_OK) return fail(rc == NFEC_ENOTSUP ? NFEC_EDEVICE : rc, "fused decode launch failed");
        gate = w.gate.p;
    }
    if ((rc = launch_rs8_bitsliced_reencode(c->k, c->m, reencode_args(c, b, r, p, fvec, gate, gen), s)))
        return fail(rc, "bit-sliced re-encode launch failed");
    if (!r.solve) return launch_gf8_matmul(stage2_gf8_args(c, b, r, p, fvec), false, s);
    // bit-sliced snippet-table solve for blocks with <= 16 erasures, the v_perm kernel for the rest
    Gf8SolveArgs a2 = solve_args(c, b, r, p, fvec, gate, gen);
    if (r.solve_bs) {
        rc = launch_gf8_solve_bs(a2, s);
        if (rc != NFEC_OK && rc != NFEC_ENOTSUP) return fail(rc, "bit-sliced solve launch failed");
        if (rc == NFEC_OK) {
            if (r.E <= 16) return NFEC_OK;
            a2.min_rows = 16;
        }
    }
    return launch_gf8_solve(a2, r.E, c->m, s);
}

// ---- RS8 on the runtime-coefficient kernel, RS8 / RS16 on the generic kernels ----
RsPlanArgs plan_args(nfec_codec* c, const nfec_block_batch* b, const DecodeRoute& r, const Pass& p)
{
    DecodeWorkspace& w = c->ws;
    RsPlanArgs a;
    a.bits = c->kind == NFEC_RS16 ? 16 : 8;
    a.k = c->k;
    a.m = c->m;
    a.nblocks = p.nb;
    a.num_data = p.nd;
    a.erasure_locs = p.locs;
    a.erasure_stride = p.lstride;
    a.erasure_counts = p.counts;
    a.gen_parity = c->d_gen.p;
    a.exp_tab = c->d_exp.p;
    a.log_tab = c->d_log.p;
    a.status = p.status;
    a.rows = w.rows.p;
    a.in_slots1 = w.islots.p;
    a.out_slots2 = w.oslots.p;
    a.cols2 = w.cols.p;
    a.coef_stride = r.dcs;
    a.coef1 = w.coef1.p;
    a.coef2 = w.coef2.p;
    a.work = r.big_plan ? w.work.p : nullptr;
    a.work_block_bytes = rs_plan_work_bytes(r.dcs, c->sym);
    if (r.cf16 || r.kind == Route::RS8_RT) {  // the closed forms' constants
        a.lwp = c->d_lwp.p;
        a.lw = c->d_lw.p;
    }
    if (r.t3dec) {
        a.rows1 = w.rows1.p;
        a.rmax = w.rmax.p;
        a.zero_base = p.blocks;
        a.zero_block_stride = b->block_stride;
        a.zero_seg_stride = b->seg_stride;
        a.zero_vec = c->vec & ~1u;
    }
    return a;
}

// closed-form plan of each block's whole repair map, then one pass of the runtime-coefficient
// kernel over the 8-byte pieces and the tail kernel over the rest
int pass_rs8_rt(nfec_codec* c, const nfec_block_batch* b, const DecodeRoute& r, const Pass& p, hipStream_t s, bool& tail)
{
    int rc;
    const Rs8RtArgs a = rt_repair_args(c, b, r, p);
    if ((r.vec8 && !rs8_rt_covers(a)) || (r.nt && !rs8_rt_tail_covers(a, r.vec8, r.nt)))
        return fail(NFEC_ENOTSUP, "runtime-coefficient repair: batch layout past its 2^31 offsets");
    if ((rc = launch_rs8_plan_rt(plan_args(c, b, r, p), r.np, s))) return rc;
    if (r.vec8 && (rc = launch_rs8_rt(a, s)))
        return fail(rc == NFEC_ENOTSUP ? NFEC_EDEVICE : rc, "runtime-coefficient repair launch failed");
    if (r.nt) {
        if ((rc = launch_rs8_rt_tail(a, r.vec8, r.nt, s)))
            return fail(rc == NFEC_ENOTSUP ? NFEC_EDEVICE : rc, "runtime-coefficient repair tail launch failed");
        tail = true;
    }
    return NFEC_OK;
}

// stage 1 on the generic kernels: z_t = parity(P_t) ^ sum_{present c} G[P_t][c] d_c -> z rows
template <typename Args>
void gather_stage1(Args& a, nfec_codec* c, const nfec_block_batch* b, const DecodeRoute& r, const Pass& p)
{
    DecodeWorkspace& w = c->ws;
    const ZView z = z_view(c, r);
    a.in_base = p.blocks;
    a.in_block_stride = b->block_stride;
    a.in_seg_stride = b->seg_stride;
    a.in_slots = w.islots.p;
    a.in_count = p.nd;
    a.cols_const = c->k;
    a.out_base = z.base;
    a.out_block_stride = z.block_stride;
    a.out_seg_stride = z.seg_stride;
    a.out_slot_mode = OUT_SLOT_ROW;
    a.row_count = r.t3dec ? w.rows1.p : w.rows.p;  // (t3dec: the blocks the product kernel left)
    a.slots_stride = c->k;
    a.coef_block_stride = (uint64_t)c->k * r.dcs;
    a.coef_col_stride = r.dcs;
    a.nblocks = p.nb;
}

// RS16 stage 2 on the exp-table kernel
Gf16MatmulArgs stage2_gf16_args(nfec_codec* c, const nfec_block_batch* b, const DecodeRoute& r, const Pass& p)
{
    DecodeWorkspace& w = c->ws;
    const ZView z = z_view(c, r);
    Gf16MatmulArgs a;
    a.in_base = z.base;
    a.in_block_stride = z.block_stride;
    a.in_seg_stride = z.seg_stride;
    a.in_count = w.cols.p;
    a.cols_const = c->k;
    a.out_base = p.blocks;
    a.out_block_stride = b->block_stride;
    a.out_seg_stride = b->seg_stride;
    a.out_slots = w.oslots.p;
    a.out_slot_mode = OUT_SLOT_LIST;
    a.row_count = w.rows.p;
    a.slots_stride = c->k;
    a.coef = reinterpret_cast<const uint16_t*>(w.coef2.p);
    a.coef_block_stride = (uint64_t)r.dcs * r.dcs;
    a.coef_col_stride = r.dcs;
    a.exp_tab = reinterpret_cast<const uint16_t*>(c->d_exp.p);
    a.log_tab = c->d_log.p;
    a.nblocks = p.nb;
    a.vec_bytes = c->vec & ~1u;
    a.accumulate = accumulates(b);
    return a;
}

// RS16 stage 2 on the tower kernel in per-block mode: the per-block tables of A^-1, then the
// product; NFEC_ENOTSUP from the product leaves stage 2 to the exp-table kernel
int stage2_tw(nfec_codec* c, const nfec_block_batch* b, const DecodeRoute& r, const Pass& p, hipStream_t s)
{
    DecodeWorkspace& w = c->ws;
    const ZView z = z_view(c, r);
    const size_t tw2_elems = gf16_tw_table_elems(r.E, r.E);
    TwDecTablesArgs d;
    d.coef2 = reinterpret_cast<const uint16_t*>(w.coef2.p);
    d.dcs = r.dcs;
    d.rows = w.rows.p;
    d.out_slots = w.oslots.p;
    d.slots_stride = c->k;
    d.seg_stride = b->seg_stride;
    d.nblocks = p.nb;
    d.M = r.E;
    d.tw = w.tw2.p;
    d.tw_block_stride = tw2_elems;
    d.row_off = w.rowoff.p;
    gf16_tw_field(d.phi, &d.lam);
    const int rc = launch_tw_dec_tables(d, s);
    if (rc) return rc;
    Gf16T3Args t;
    t.base = z.base;
    t.block_stride = z.block_stride;
    t.seg_stride = z.seg_stride;
    t.nblocks = p.nb;
    t.k = r.E;
    t.m = r.E;
    t.vec_bytes = c->vec & ~1u;
    t.tw = w.tw2.p;
    t.tw_block_stride = tw2_elems;
    t.blk_rows = w.rows.p;
    t.row_off = w.rowoff.p;
    t.row_off_stride = r.E + 12;
    t.out_base = p.blocks;
    t.out_block_stride = b->block_stride;
    t.out_seg_stride = b->seg_stride;
    return launch_gf16_tw_encode(t, s);
}

// Gauss-Jordan or closed-form plan, then stage 1 (RS16 with t3dec: the product kernel for the
// blocks it takes, whose z rows the gather stage leaves alone; the gather kernel for the rest)
// and stage 2 (RS16 with tw2: the tower kernel; else the generic kernel)
int pass_rs_generic(nfec_codec* c, const nfec_block_batch* b, const DecodeRoute& r, const Pass& p, hipStream_t s, bool& tail)
{
    DecodeWorkspace& w = c->ws;
    int rc;
    if (r.t3dec) NFEC_HIP(hipMemsetAsync(w.rmax.p, 0, sizeof(uint32_t), s));
    if ((rc = launch_rs_plan(plan_args(c, b, r, p), s))) return rc;
    if (r.t3dec) {
        // z_t for t below the plan's largest such e; the gather stage then overwrites the z
        // rows of the other blocks
        rc = launch_rs16_product(c, t3_stage1_args(c, b, r, p.blocks, p.nb), s);
        if (rc == NFEC_ENOTSUP) return fail(rc, "t3 decode stage 1: layout not covered");
        if (rc) return rc;
    }
    if (c->kind == NFEC_RS8) {
        Gf8MatmulArgs a;
        gather_stage1(a, c, b, r, p);
        a.coef = w.coef1.p;
        a.vtab = c->d_vtab.p;
        a.vec_bytes = c->vec;
        if ((rc = launch_gf8_matmul(a, false, s))) return rc;
        return launch_gf8_matmul(stage2_gf8_args(c, b, r, p, c->vec), false, s);
    }
    Gf16MatmulArgs a;
    gather_stage1(a, c, b, r, p);
    a.coef = reinterpret_cast<const uint16_t*>(w.coef1.p);
    a.exp_tab = reinterpret_cast<const uint16_t*>(c->d_exp.p);
    a.log_tab = c->d_log.p;
    a.vec_bytes = c->vec & ~1u;
    if ((rc = launch_gf16_matmul(a, s))) return rc;
    if (r.tw2 && (rc = stage2_tw(c, b, r, p, s)) != NFEC_ENOTSUP) return rc;
    return launch_gf16_matmul(stage2_gf16_args(c, b, r, p), s);
}

// ---- decode on a device batch ----
int decode_device_impl(nfec_codec* c, const nfec_block_batch* b, const uint16_t* locs, uint32_t lstride,
                       const uint16_t* counts, int32_t* status, hipStream_t s, bool caller_locked, int& path, bool& tail)
{
    if (!locs || !counts) return fail(NFEC_EINVAL, "null erasure arrays");
    if (c->kind == NFEC_MDP && accumulates(b)) return fail(NFEC_ENOTSUP, "MDP decode requires zero-filled erased segments");
    std::unique_lock<std::mutex> lk(c->mu, std::defer_lock);
    if (!caller_locked) lk.lock();
    DecodeRoute r = decode_route(c, b);
    path = r.dpath;
    if (r.kind == Route::RS16_TOWER) return decode_rs16_tw(c, b, locs, lstride, counts, status, s);
    const uint32_t sb = decode_pass_size(c, r, b->nblocks);
    decode_route_stage1(c, b, r, sb);
    int rc;
    if ((rc = decode_reserve(c, r, sb, status != nullptr))) return rc;
    for (uint32_t b0 = 0; b0 < b->nblocks; b0 += sb) {
        const Pass p{static_cast<uint8_t*>(b->blocks) + (uint64_t)b0 * b->block_stride,
                     std::min(sb, b->nblocks - b0),
                     b->num_data ? b->num_data + b0 : nullptr,
                     locs + (uint64_t)b0 * lstride,
                     counts + b0,
                     lstride,
                     status ? status + b0 : c->ws.status.p};
        switch (r.kind) {
        case Route::MDP_RT:
        case Route::MDP_SOLVE: rc = pass_mdp(c, b, r, p, s, tail); break;
        case Route::RS8_FIXED: rc = pass_rs8_fixed(c, b, r, p, s, tail); break;
        case Route::RS8_RT: rc = pass_rs8_rt(c, b, r, p, s, tail); break;
        default: rc = pass_rs_generic(c, b, r, p, s, tail); break;
        }
        if (rc) return rc;
    }
    return NFEC_OK;
}

}  // namespace

// counts each batch decode by the path that took it (nfec_codec_decode_paths)
int nfec::decode_device(nfec_codec* c, const nfec_block_batch* b, const uint16_t* locs, uint32_t lstride,
                        const uint16_t* counts, int32_t* status, hipStream_t s, bool caller_locked)
{
    int path = NFEC_DPATH_GENERIC;
    bool tail = false;
    const int rc = decode_device_impl(c, b, locs, lstride, counts, status, s, caller_locked, path, tail);
    if (rc == NFEC_OK) c->dec_paths[path].fetch_add(1, std::memory_order_relaxed);
    if (rc == NFEC_OK && tail) c->tail_batches[1].fetch_add(1, std::memory_order_relaxed);
    return rc;
}
