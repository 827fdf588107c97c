// nfec_api.cpp -- C ABI (include/nfec.h): codec objects and batch orchestration.
//
// A codec mirrors one NormEncoder/NormDecoder Init (reference normEncoderRS8.cpp:400-462,
// :542-649; normEncoderRS16.cpp:399-461; normEncoderMDP.cpp:56-84): it owns the generator
// (built once on the host, uploaded to HBM) and the per-value kernel tables.  Batched calls
// only enqueue kernels on the caller's stream; no host<->device traffic on the hot path.
// The codec object is in codec_state.hpp; which kernels a device batch reaches is decided in
// dispatch_encode.cpp and dispatch_decode.cpp; the host-resident batches are in host_pipeline.cpp.
#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <deque>
#include <functional>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <thread>
#include <chrono>
#include <vector>

#include "bitslice.hpp"
#include "codec_state.hpp"
#include "nack_layout.hpp"
#include "rx_parse.hpp"

using namespace nfec;

namespace {

int upload(DevBuf<uint8_t>& d, const void* src, size_t bytes)
{
    int rc = d.reserve(bytes);
    if (rc) return rc;
    NFEC_HIP(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
    return NFEC_OK;
}

}  // namespace

namespace nfec {

int host_only_fail()
{
    return fail(NFEC_EDEVICE, "host-only codec (NFEC_OPT_HOST_ONLY): no GPU path");
}

int check_batch(const nfec_codec* c, const nfec_block_batch* b)
{
    if (!c || !b) return fail(NFEC_EINVAL, "null codec or batch");
    if (c->host_only) return host_only_fail();
    if (b->nblocks == 0) return NFEC_OK;
    if (!b->blocks) return fail(NFEC_EINVAL, "null blocks pointer");
    if ((reinterpret_cast<uintptr_t>(b->blocks) & 7) || (b->seg_stride & 7) || (b->block_stride & 7))
        return fail(NFEC_EINVAL, "blocks, seg_stride and block_stride must be multiples of 8 bytes");
    if (b->seg_stride < c->vec) return fail(NFEC_EINVAL, "seg_stride < vector_size");
    if (b->block_stride < (uint64_t)(c->k + c->m) * b->seg_stride && b->nblocks > 1)
        return fail(NFEC_EINVAL, "block_stride smaller than (k+m)*seg_stride");
    return NFEC_OK;
}

// NFEC_GF16_T3=0 disables the shared-table RS16 encode (A/B runs, diagnostic library)
bool use_gf16_t3()
{
    static const bool v = diag_knob("NFEC_GF16_T3", 1) != 0;
    return v;
}

// RS16 products through the tower field (gen_gf16_tw.hip, the default since round 3) or the
// shared LDS tables (gen_gf16_t3.hip, NFEC_OPT_RS16_SHARED_TABLES: both are exact, the tests run
// both); chosen per codec, so one process can hold codecs of both kinds.  NFEC_RS16_TW=0/1
// overrides (diagnostic library).
bool use_gf16_tw(const nfec_codec* c)
{
    return diag_knob("NFEC_RS16_TW", (c->opts & NFEC_OPT_RS16_SHARED_TABLES) ? 0 : 1) != 0;
}

}  // namespace nfec

namespace {

// ---- codec construction ----
// log W'(x_j) over the k source points and log W(y_p) at the parity points: the constants of
// the closed-form plans (rs_plan2_kernel for RS8, rs16_plan_cf_kernel for RS16, the host repair)
// The closed-form plans' constants: log W'(x_j) = sum_{l != j, l < k} log(x_j + x_l) over the
// source points and log W(y_p) = sum_{l < k} log(y_p + x_l) at the parity points, with x_0 = 0,
// x_l = alpha^(l-1), y_p = alpha^(k+p-1) (normEncoderRS8.cpp:432-439).  Since
// alpha^a + alpha^b = alpha^a (1 + alpha^(b-a)), with g(d) = log(1 + alpha^d):
//   log W'(x_0)  = sum_{l=1}^{k-1} (l - 1) = (k-1)(k-2)/2
//   log W'(x_j)  = (k-1)(j-1) + sum_{d=1-j, d != 0}^{k-1-j} g(d)          (j >= 1)
//   log W(y_p)   = (k+p-1) + (k-1)(k-2)/2 + sum_{d=p+1}^{k+p-1} g(d)
// so one prefix sum of g over d in [-(k-2), k+m-2] gives all of them in O(k + m) (the direct
// sums are O(k^2 + mk): seconds at RS16's largest k).  Every d stays inside (-q, q) and is never
// 0 mod q, so 1 + alpha^d is never zero.
static void plan_constants(nfec_codec* c, const Field& f)
{
    const int64_t k = c->k, m = c->m, q = f.q;
    const int64_t lo = -(k - 2), hi = k + m - 2;  // the d range (lo <= 0 <= hi for k >= 2)
    std::vector<int64_t> pre((size_t)std::max<int64_t>(0, hi - lo + 2), 0);  // pre[i] = sum of g over [lo, lo + i)
    for (int64_t d = lo, i = 0; d <= hi; ++d, ++i) {
        const int64_t g = d == 0 ? 0 : (int64_t)f.log[1u ^ f.exp[(uint32_t)(((d % q) + q) % q)]];
        pre[(size_t)i + 1] = pre[(size_t)i] + g;
    }
    auto sum = [&](int64_t a, int64_t b) -> int64_t {  // g over [a, b] (d = 0 counts 0)
        if (b < a) return 0;
        return pre[(size_t)(b - lo + 1)] - pre[(size_t)(a - lo)];
    };
    std::vector<uint16_t> lwp(c->k), lw(c->m);
    const int64_t tri = (k - 1) * (k - 2) / 2;
    for (int64_t j = 0; j < k; ++j) {
        const int64_t v = j == 0 ? tri : (k - 1) * (j - 1) + sum(1 - j, k - 1 - j);
        lwp[(size_t)j] = (uint16_t)(v % q);
    }
    for (int64_t p = 0; p < m; ++p) lw[(size_t)p] = (uint16_t)(((k + p - 1) + tri + sum(p + 1, k + p - 1)) % q);
    c->h_lwp = lwp;
    c->h_lw = lw;
}

int build_codec(nfec_codec* c)
{
    const bool wide = c->kind == NFEC_RS16;
    c->sym = wide ? 2 : 1;
    c->cs = round_up(std::max(c->m, 1u), kRowPad);
    const Field& f = wide ? gf16() : gf8();
    if (c->host_only) {
        // what the host per-call paths read: the generator (MDP: the polynomial and the full
        // block's LFSR map) and the closed-form plan constants
        if (c->kind == NFEC_MDP) {
            if (c->k + c->m > 255 || c->m == 0) return fail(NFEC_ERANGE, "MDP: numData + numParity > 255");
            mdp_generator_poly(c->m, c->mdp_g);
            std::vector<uint8_t> map((size_t)c->m * c->k);
            mdp_encode_matrix(c->mdp_g, c->m, c->k, map.data());
            c->gen.assign(map.begin(), map.end());
            return NFEC_OK;
        }
        if (rs_generator(wide ? 16 : 8, c->k, c->m, c->gen)) return fail(NFEC_ERANGE, "RS: numData/numParity exceeds code limits");
        plan_constants(c, f);  // any shape: the host repair's closed form has no size limit
        return NFEC_OK;
    }
    if (c->kind == NFEC_MDP) {
        if (c->k + c->m > 255 || c->m == 0) return fail(NFEC_ERANGE, "MDP: numData + numParity > 255");
        std::vector<uint8_t> g;
        mdp_generator_poly(c->m, g);
        c->mdp_g = g;
        // encode matrices for every block length nd = 1..k: [nd-1][col][cs]
        std::vector<uint8_t> coef((size_t)c->k * c->k * c->cs, 0);
        std::vector<uint8_t> map((size_t)c->m * c->k);
        for (uint32_t nd = 1; nd <= c->k; ++nd) {
            mdp_encode_matrix(g, c->m, nd, map.data());
            for (uint32_t col = 0; col < nd; ++col)
                for (uint32_t r = 0; r < c->m; ++r)
                    coef[((size_t)(nd - 1) * c->k + col) * c->cs + r] = map[(size_t)r * nd + col];
            if (nd == c->k) {
                c->gen.assign(map.begin(), map.end());
            }
        }
        int rc = upload(c->d_coef, coef.data(), coef.size());
        if (rc) return rc;
        {
            // the same block maps as runtime-coefficient tables, one per nd (shortened encodes)
            const uint32_t cs = rs8_rt_col_stride(c->m) / 2;
            c->rt_block_bytes = (uint64_t)c->k * cs * 2;
            // (+ padding: the kernel's scalar-cache touch reads up to 4 columns past an entry)
            std::vector<uint16_t> t((size_t)c->k * c->k * cs + 4 * cs + 64, 0);
            for (uint32_t nd = 1; nd <= c->k; ++nd)
                for (uint32_t col = 0; col < nd; ++col)
                    for (uint32_t r = 0; r < c->m; ++r)
                        t[((size_t)(nd - 1) * c->k + col) * cs + r] =
                            (uint16_t)(coef[((size_t)(nd - 1) * c->k + col) * c->cs + r] << 7);
            if ((rc = c->d_rt.reserve(t.size()))) return rc;
            NFEC_HIP(hipMemcpy(c->d_rt.p, t.data(), t.size() * 2, hipMemcpyHostToDevice));
        }
        // one in-order Encode step: inputs [d, P0..P(m-1)] -> new P (normEncoderMDP.cpp:178-211)
        std::vector<uint8_t> step((size_t)(c->m + 1) * c->cs, 0);
        for (uint32_t i = 0; i < c->m; ++i) {
            const uint8_t gi = (i + 1 < c->m) ? g[c->m - 1 - i] : g[0];
            step[(size_t)0 * c->cs + i] = gi;              // data
            step[(size_t)1 * c->cs + i] ^= gi;             // P0 enters the feedback
            if (i + 1 < c->m) step[(size_t)(i + 2) * c->cs + i] ^= 1;  // shift P(i+1) -> P(i)
        }
        rc = upload(c->d_mdp_step, step.data(), step.size());
        if (rc) return rc;
    } else {
        const int bits = wide ? 16 : 8;
        int rc = rs_generator(bits, c->k, c->m, c->gen);
        if (rc) return fail(rc, "RS: numData/numParity exceeds code limits");
        std::vector<uint8_t> coef((size_t)c->k * c->cs * c->sym, 0);
        std::vector<uint8_t> genb((size_t)c->m * c->k * c->sym);
        for (uint32_t p = 0; p < c->m; ++p)
            for (uint32_t j = 0; j < c->k; ++j) {
                const uint32_t v = c->gen[(size_t)p * c->k + j];
                if (wide) {
                    reinterpret_cast<uint16_t*>(coef.data())[(size_t)j * c->cs + p] = (uint16_t)v;
                    reinterpret_cast<uint16_t*>(genb.data())[(size_t)p * c->k + j] = (uint16_t)v;
                } else {
                    coef[(size_t)j * c->cs + p] = (uint8_t)v;
                    genb[(size_t)p * c->k + j] = (uint8_t)v;
                }
            }
        rc = upload(c->d_coef, coef.data(), coef.size());
        if (rc) return rc;
        rc = upload(c->d_gen, genb.data(), genb.size());
        if (rc) return rc;
        if (!wide) {
            const std::vector<uint16_t> t = rs8_rt_table(c->gen, c->k, c->m);
            if ((rc = c->d_rt.reserve(t.size()))) return rc;
            NFEC_HIP(hipMemcpy(c->d_rt.p, t.data(), t.size() * 2, hipMemcpyHostToDevice));
        }
        // RS16: table offsets of the bit-sliced encode, 128 bytes per coefficient.  Every wave
        // re-reads its rows' offsets per column, so the kernel only wins while the table stays
        // cache-resident: (400, 100) is 5.3 MB and 11 % faster than the exp-table kernel,
        // (4096, 256) is 134 MB and 5 % slower.  Larger codes keep the
        // exp-table kernel.
        if (wide && (uint64_t)c->k * gf16_bs_rows_padded(c->m) * 128 <= (16ull << 20)) {
            std::vector<uint16_t> sel((size_t)c->k * gf16_bs_rows_padded(c->m) * 64);
            gf16_bs_selectors(c->gen, c->k, c->m, sel.data());
            if ((rc = c->d_sel16.reserve(sel.size()))) return rc;
            NFEC_HIP(hipMemcpy(c->d_sel16.p, sel.data(), sel.size() * 2, hipMemcpyHostToDevice));
        }
        // RS16: LDS offsets of the shared-table encode (gen_gf16_t3.hip), 96 bytes per
        // coefficient (C4, k = 4096, m = 256: 104 MB)
        if (wide && use_gf16_t3() && use_gf16_tw(c)) {
            std::vector<uint16_t> off(gf16_tw_table_elems(c->k, c->m));
            gf16_tw_offsets(c->gen, c->k, c->m, off.data());
            if ((rc = c->d_twoff.reserve(off.size()))) return rc;
            NFEC_HIP(hipMemcpy(c->d_twoff.p, off.data(), off.size() * 2, hipMemcpyHostToDevice));
            c->tw = true;
        } else if (wide && use_gf16_t3()) {
            const uint32_t mp = gf16_t3_rows_padded(c->m);
            std::vector<uint16_t> off((size_t)(c->k + 1) * mp * 48);
            gf16_t3_offsets(c->gen, c->k, c->m, off.data());
            if ((rc = c->d_t3off.reserve(off.size()))) return rc;
            NFEC_HIP(hipMemcpy(c->d_t3off.p, off.data(), off.size() * 2, hipMemcpyHostToDevice));
        }
        // RS16: the Toeplitz split of the generator, three (m/2)-row products over k/2 columns
        // (one Karatsuba level) or, on the tower kernel, nine (m/4)-row products over k/4 columns
        // (two levels) instead of one m-row product over k (kernels_tmvp.hip), where its passes
        // are fewer: NFEC_OPT_RS16_TOEPLITZ_OFF never, NFEC_OPT_RS16_TOEPLITZ_ON whenever the
        // shape allows it, at the most levels allowed (tests), neither when it pays;
        // NFEC_OPT_RS16_TOEPLITZ_ONE_LEVEL caps it at one level (NFEC_RS16_TMVP=0/1/-1 overrides,
        // diagnostic library)
        // (a vector size not a multiple of 8: the split over its 8-byte pieces, the tail kernel
        // over the last 2-6 bytes with the whole generator; tower kernel only)
        if (wide && use_gf16_t3() && ((c->vec % 8) == 0 || (c->tw && c->vec >= 8))) {
            const int mode = (int)diag_knob("NFEC_RS16_TMVP",
                                            (c->opts & NFEC_OPT_RS16_TOEPLITZ_OFF)  ? 0
                                            : (c->opts & NFEC_OPT_RS16_TOEPLITZ_ON) ? 1
                                                                                    : -1,
                                            -1, 1);
            const uint32_t rpp = kGf16T3RowsPerPass;
            // cost of each form per block, in the products' units (about one column step per
            // pass, weighted on the tower kernel by the cost of a pass of the configuration a
            // launch of that many rows takes, gf16_tw_cost): the products (3^L of m >> L rows
            // over k >> L columns, plus ~20 columns' worth of fixed work per pass), the prescale
            // (~165 per column it moves: it is HBM-bound) and the postscale (per parity row ~460
            // at one level, ~700 at two: its constant multiplies).  Fitted to the split forced
            // at 0 / 1 / 2 levels on (128, 32), (256, 64), (512, 128) and C4
            // (profiles/r05/tmvp_levels/: fastest at 0, 0, 2 and 2 levels).  A third level
            // measured slower: its prescale moves 3.4 k columns per block against 2.25 k.
            const int max_levels = (!c->tw || (c->opts & NFEC_OPT_RS16_TOEPLITZ_ONE_LEVEL)) ? 1 : 2;
            uint64_t cost[3];
            int top = 0;
            for (int L = 0; L <= 2; ++L) {
                cost[L] = ~0ull;
                const uint32_t r = c->m >> L;
                if (L > max_levels || r == 0 || (L && (c->m % (1u << L)))) continue;
                // (the shared-table kernel's column map needs chunks of a power of two)
                if (L && !c->tw && ((c->m / 2) & (c->m / 2 - 1))) continue;
                top = L;
                uint64_t np = 1;
                for (int i = 0; i < L; ++i) np *= 3;
                const uint64_t cols = (c->k >> L) + 20;
                const uint64_t prod_cost = c->tw ? np * gf16_tw_cost(r) * cols : np * ((r + rpp - 1) / rpp) * cols;
                // (the shared-table kernel keeps the round-2 rule: passes alone)
                cost[L] = prod_cost + (!c->tw ? 0ull
                                       : L == 1 ? 165ull * (c->k + c->k / 2) + 460ull * c->m
                                       : L == 2 ? 165ull * (c->k + c->k / 2 + 3ull * (c->k / 4)) + 700ull * c->m
                                                : 0ull);
            }
            int levels = 0;
            if (mode == 1) levels = top;
            else if (mode != 0)
                for (int L = 1; L <= 2; ++L)
                    if (cost[L] < cost[levels]) levels = L;
            uint32_t nprod = 1;
            for (int i = 0; i < levels; ++i) nprod *= 3;
            std::vector<uint32_t> prod[9];
            std::vector<uint16_t> cm, wm, gm;
            if (levels && rs16_tmvp_plan_levels(c->k, c->m, c->gen, levels, prod, cm, wm, gm)) {
                const uint32_t cols = c->k >> levels, rows = c->m >> levels;
                const uint32_t mp = gf16_t3_rows_padded(rows);
                const size_t one = c->tw ? gf16_tw_table_elems(cols, rows) : (size_t)(cols + 1) * mp * 48;
                std::vector<uint16_t> off(nprod * one);
                for (uint32_t e = 0; e < nprod; ++e) {
                    if (c->tw) gf16_tw_offsets(prod[e], cols, rows, off.data() + e * one);
                    else gf16_t3_offsets(prod[e], cols, rows, off.data() + e * one);
                }
                std::vector<uint16_t> mat;
                mat.insert(mat.end(), cm.begin(), cm.end());
                mat.insert(mat.end(), wm.begin(), wm.end());
                mat.insert(mat.end(), gm.begin(), gm.end());
                DevBuf<uint16_t>& dst = c->tw ? c->d_tmvp_tw : c->d_tmvp_off;
                if ((rc = dst.reserve(off.size()))) return rc;
                if ((rc = c->d_tmvp_mat.reserve(mat.size()))) return rc;
                NFEC_HIP(hipMemcpy(dst.p, off.data(), off.size() * 2, hipMemcpyHostToDevice));
                NFEC_HIP(hipMemcpy(c->d_tmvp_mat.p, mat.data(), mat.size() * 2, hipMemcpyHostToDevice));
                NFEC_HIP(hipEventCreateWithFlags(&c->tmvp_done, hipEventDisableTiming));
                c->tmvp = true;
                c->tmvp_levels = levels;
            }
        }
        plan_constants(c, f);  // the host repair (nfec_decode_vectors_host) takes any shape
        if (!wide || std::min(c->k, c->m) <= kPlanCfMaxE) {
            if ((rc = c->d_lwp.reserve(c->k))) return rc;
            if ((rc = c->d_lw.reserve(c->m))) return rc;
            NFEC_HIP(hipMemcpy(c->d_lwp.p, c->h_lwp.data(), c->h_lwp.size() * 2, hipMemcpyHostToDevice));
            NFEC_HIP(hipMemcpy(c->d_lw.p, c->h_lw.data(), c->h_lw.size() * 2, hipMemcpyHostToDevice));
        }
    }
    // field tables
    if (wide) {
        std::vector<uint16_t> ex(2 * f.q), lg(f.q + 1);
        for (uint32_t i = 0; i < 2 * f.q; ++i) ex[i] = (uint16_t)f.exp[i];
        for (uint32_t i = 0; i <= f.q; ++i) lg[i] = (uint16_t)f.log[i];
        int rc = upload(c->d_exp, ex.data(), ex.size() * 2);
        if (rc) return rc;
        rc = c->d_log.reserve(lg.size());
        if (rc) return rc;
        NFEC_HIP(hipMemcpy(c->d_log.p, lg.data(), lg.size() * 2, hipMemcpyHostToDevice));
    } else {
        std::vector<uint8_t> ex(2 * f.q);
        std::vector<uint16_t> lg(f.q + 1);
        for (uint32_t i = 0; i < 2 * f.q; ++i) ex[i] = (uint8_t)f.exp[i];
        for (uint32_t i = 0; i <= f.q; ++i) lg[i] = (uint16_t)f.log[i];
        int rc = upload(c->d_exp, ex.data(), ex.size());
        if (rc) return rc;
        rc = c->d_log.reserve(lg.size());
        if (rc) return rc;
        NFEC_HIP(hipMemcpy(c->d_log.p, lg.data(), lg.size() * 2, hipMemcpyHostToDevice));
        std::vector<uint32_t> vt(256 * 8);
        for (uint32_t v = 0; v < 256; ++v) vperm_table(v, &vt[v * 8]);
        rc = c->d_vtab.reserve(vt.size());
        if (rc) return rc;
        NFEC_HIP(hipMemcpy(c->d_vtab.p, vt.data(), vt.size() * 4, hipMemcpyHostToDevice));
    }
    return NFEC_OK;
}

}  // namespace

namespace nfec {

// NFEC_FORCE_GENERIC=1 disables the generated bit-sliced kernels (A/B runs, diagnostic library)
bool force_generic()
{
    static const bool v = diag_knob("NFEC_FORCE_GENERIC", 0) != 0;
    return v;
}

// whether the generated bit-sliced kernels cover this RS8 shape (cached per shape; codecs on
// other host threads ask concurrently, so the answer is computed into a per-call buffer under
// a lock, never into shared scratch -- the reference's unlocked fec_initialized race,
// normEncoderRS8.cpp:379-388, is not reintroduced)
bool has_bitsliced(uint32_t k, uint32_t m)
{
    static std::mutex mu;
    static std::map<uint32_t, bool> known;
    const uint32_t key = (k << 16) | m;
    std::lock_guard<std::mutex> lk(mu);
    auto it = known.find(key);
    if (it != known.end()) return it->second;
    std::vector<uint8_t> scratch(256 * 256);
    const bool v = bitsliced_encode_generator(k, m, scratch.data()) == NFEC_OK;
    known.emplace(key, v);
    return v;
}

// tuning knobs of the bit-sliced kernels (A/B runs): bit 0 XCD-contiguous workgroup
// mapping (default on: neighbouring item groups share the 128-byte lines at their boundaries,
// so one XCD's L2 fetches them once; encode 2.38 -> 2.35 ms), bit 1 nontemporal parity stores
uint32_t bs_flags()
{
    static const uint32_t f = (uint32_t)diag_knob("NFEC_BS_FLAGS", 1, 0, 3);
    return f;
}

// NFEC_Q4=0 (diagnostic library) replaces the 4-role-wave encode kernels (gen_rs8_q4.hip) by
// the round-1 2-role assembly kernels, which only the diagnostic library builds
bool use_q4()
{
    static const bool v = diag_knob("NFEC_Q4", 1) != 0;
    return v;
}

// NFEC_ASM=0 (diagnostic library): compiler-allocated bit-sliced kernels only
bool use_asm()
{
    static const bool v = diag_knob("NFEC_ASM", 1) != 0;
    return v;
}

}  // namespace nfec

// =====================================================================================
// C ABI
// =====================================================================================
extern "C" {

int nfec_abi_version(void) { return NFEC_ABI_VERSION; }

const char* nfec_last_error(void) { return last_error_cstr(); }

int nfec_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    int good = 0;
    for (int d = 0; d < n; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0)
            ++good;
    }
    return good;
}

}  // extern "C"

namespace {

int create_one(int device, int kind, uint32_t num_data, uint32_t num_parity, uint32_t vector_size, uint32_t opts,
               nfec_codec** out)
{
    if (opts & NFEC_OPT_HOST_ONLY) {
        // no device is touched: Init's math and the host per-call paths only
        std::unique_ptr<nfec_codec> c(new nfec_codec);
        c->kind = kind;
        c->device = -1;
        c->opts = opts;
        c->k = num_data;
        c->m = num_parity;
        c->vec = vector_size;
        c->host_only = true;
        c->async.device = -1;
        const int rc = build_codec(c.get());
        if (rc) return rc;
        *out = c.release();
        return NFEC_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        (void)hipGetLastError();
        return fail(NFEC_EDEVICE, "no such HIP device (the MI355X path needs a GPU)");
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(NFEC_EDEVICE, "device is not gfx950 (MI355X)");
    DeviceGuard g(device);
    if (!g.ok) return fail(NFEC_EDEVICE, "hipSetDevice failed");
    std::unique_ptr<nfec_codec> c(new nfec_codec);
    c->kind = kind;
    c->device = device;
    c->opts = opts;
    c->k = num_data;
    c->m = num_parity;
    c->vec = vector_size;
    c->async.device = device;  // fixed before any worker thread can read it
    int rc = build_codec(c.get());
    if (rc) return rc;
    *out = c.release();
    return NFEC_OK;
}

// the stripe whose device holds a device batch (a single-device codec: itself).  Only device
// allocations name a device: a batch in host-mapped or registered host memory (which the GPU
// reads over PCIe, as a single-device codec would pass it through) or in memory HIP does not
// know runs on the first stripe, so a codec's device list does not change which batches it takes.
nfec_codec* stripe_for(nfec_codec* c, const void* dev_ptr)
{
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof(at));
    // memory HIP does not know (plain pageable malloc: the query fails or reports it
    // unregistered) is refused -- a kernel dereferencing unmapped host memory faults the GPU
    // (no XNACK); pinned / registered host and managed memory runs on stripe 0
    if (hipPointerGetAttributes(&at, dev_ptr) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    if (at.type != hipMemoryTypeHost && at.type != hipMemoryTypeManaged && at.type != hipMemoryTypeUnified &&
        at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeArray)
        return nullptr;
    // a one-device codec runs any memory HIP maps (its own device's, a peer's, pinned host)
    if (c->stripes.empty()) return c;
    if (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeArray) return c->stripes[0].get();
    for (auto& st : c->stripes)
        if (st->device == at.device) return st.get();
    return nullptr;
}

}  // namespace

extern "C" {

int nfec_codec_create(int device, int kind, uint32_t num_data, uint32_t num_parity, uint32_t vector_size,
                      nfec_codec** out)
{
    nfec_codec_config cfg{};
    cfg.kind = kind;
    cfg.num_data = num_data;
    cfg.num_parity = num_parity;
    cfg.vector_size = vector_size;
    const int32_t dev = device;
    cfg.devices = &dev;
    cfg.num_devices = 1;
    return nfec_codec_create_ex(&cfg, out);
}

int nfec_codec_create_ex(const nfec_codec_config* cfg, nfec_codec** out)
{
    if (!out || !cfg) return fail(NFEC_EINVAL, "null argument");
    *out = nullptr;
    const int kind = cfg->kind;
    if (kind != NFEC_RS8 && kind != NFEC_RS16 && kind != NFEC_MDP) return fail(NFEC_EINVAL, "unknown codec kind");
    if (cfg->num_data == 0 || cfg->num_parity == 0) return fail(NFEC_EINVAL, "numData and numParity must be > 0");
    if (cfg->vector_size == 0 || cfg->vector_size > 65535) return fail(NFEC_EINVAL, "vectorSize must be in [1, 65535]");
    if (cfg->flags & ~(uint32_t)(NFEC_OPT_RS16_SHARED_TABLES | NFEC_OPT_RS16_TOEPLITZ_OFF | NFEC_OPT_RS16_TOEPLITZ_ON |
                                 NFEC_OPT_HOST_ONLY | NFEC_OPT_RS16_TOEPLITZ_ONE_LEVEL))
        return fail(NFEC_EINVAL, "unknown option flag");
    if ((cfg->flags & NFEC_OPT_HOST_ONLY) && cfg->num_devices > 1)
        return fail(NFEC_EINVAL, "a host-only codec takes no device list");
    if ((cfg->flags & NFEC_OPT_RS16_TOEPLITZ_OFF) && (cfg->flags & NFEC_OPT_RS16_TOEPLITZ_ON))
        return fail(NFEC_EINVAL, "Toeplitz split both on and off");
    const uint32_t nd = cfg->num_devices ? cfg->num_devices : 1;
    if (nd > 64) return fail(NFEC_EINVAL, "more than 64 devices");
    if (cfg->num_devices > 0 && !cfg->devices) return fail(NFEC_EINVAL, "null device list");
    auto dev_at = [&](uint32_t i) { return cfg->devices ? (int)cfg->devices[i] : 0; };
    if (nd == 1) return create_one(dev_at(0), kind, cfg->num_data, cfg->num_parity, cfg->vector_size, cfg->flags, out);
    std::unique_ptr<nfec_codec> c(new nfec_codec);
    for (uint32_t i = 0; i < nd; ++i) {
        nfec_codec* one = nullptr;
        const int rc = create_one(dev_at(i), kind, cfg->num_data, cfg->num_parity, cfg->vector_size, cfg->flags, &one);
        if (rc) return rc;  // the stripes built so far go with c
        c->stripes.emplace_back(one);
    }
    const nfec_codec* s0 = c->stripes[0].get();
    c->kind = kind;
    c->device = s0->device;
    c->opts = cfg->flags;
    c->k = s0->k;
    c->m = s0->m;
    c->vec = s0->vec;
    c->sym = s0->sym;
    c->cs = s0->cs;
    c->gen = s0->gen;
    c->async.device = s0->device;
    *out = c.release();
    return NFEC_OK;
}

int nfec_codec_num_devices(const nfec_codec* c, int32_t* devices, uint32_t cap)
{
    if (!c) return fail(NFEC_EINVAL, "null argument");
    const uint32_t n = c->stripes.empty() ? 1u : (uint32_t)c->stripes.size();
    for (uint32_t i = 0; i < n && devices && i < cap; ++i) devices[i] = c->stripes.empty() ? c->device : c->stripes[i]->device;
    return (int)n;
}

void nfec_codec_destroy(nfec_codec* codec) { delete codec; }

int nfec_build_generator(int kind, uint32_t num_data, uint32_t num_parity, void* host_out, size_t bytes)
{
    if (!host_out || num_data == 0 || num_parity == 0) return fail(NFEC_EINVAL, "bad argument");
    const size_t cnt = (size_t)num_data * num_parity;
    if (kind == NFEC_MDP) {
        if (num_data + num_parity > 255) return fail(NFEC_ERANGE, "MDP: numData + numParity > 255");
        if (bytes < cnt) return fail(NFEC_EINVAL, "output buffer too small");
        std::vector<uint8_t> g;
        mdp_generator_poly(num_parity, g);
        mdp_encode_matrix(g, num_parity, num_data, static_cast<uint8_t*>(host_out));
        return NFEC_OK;
    }
    if (kind != NFEC_RS8 && kind != NFEC_RS16) return fail(NFEC_EINVAL, "unknown codec kind");
    const size_t sym = kind == NFEC_RS16 ? 2 : 1;
    if (bytes < cnt * sym) return fail(NFEC_EINVAL, "output buffer too small");
    std::vector<uint32_t> rows;
    int rc = rs_generator(kind == NFEC_RS16 ? 16 : 8, num_data, num_parity, rows);
    if (rc) return fail(rc, "numData/numParity exceeds code limits");
    for (size_t i = 0; i < cnt; ++i) {
        if (sym == 2) static_cast<uint16_t*>(host_out)[i] = (uint16_t)rows[i];
        else static_cast<uint8_t*>(host_out)[i] = (uint8_t)rows[i];
    }
    return NFEC_OK;
}

int nfec_codec_get_info(const nfec_codec* c, nfec_codec_info* out)
{
    if (!c || !out) return fail(NFEC_EINVAL, "null argument");
    out->kind = c->kind;
    out->device = c->device;
    out->num_data = c->k;
    out->num_parity = c->m;
    out->vector_size = c->vec;
    out->symbol_bytes = c->sym;
    return NFEC_OK;
}

int nfec_codec_features(const nfec_codec* c)
{
    if (!c) return fail(NFEC_EINVAL, "null argument");
    const nfec_codec* p = primary(c);
    return (p->tmvp ? NFEC_FEATURE_RS16_TOEPLITZ : 0) | (p->tmvp_levels == 2 ? NFEC_FEATURE_RS16_TOEPLITZ2 : 0);
}

int nfec_codec_encode_paths(const nfec_codec* c, uint64_t* counts, uint32_t n)
{
    if (!c || (!counts && n)) return fail(NFEC_EINVAL, "null argument");
    for (uint32_t i = 0; i < n; ++i) {
        uint64_t v = i < NFEC_PATH_COUNT ? c->enc_paths[i].load(std::memory_order_relaxed) : 0;
        for (const auto& st : c->stripes) v += i < NFEC_PATH_COUNT ? st->enc_paths[i].load(std::memory_order_relaxed) : 0;
        counts[i] = v;
    }
    return NFEC_PATH_COUNT;
}

int nfec_codec_decode_paths(const nfec_codec* c, uint64_t* counts, uint32_t n)
{
    if (!c || (!counts && n)) return fail(NFEC_EINVAL, "null argument");
    for (uint32_t i = 0; i < n; ++i) {
        uint64_t v = i < NFEC_DPATH_COUNT ? c->dec_paths[i].load(std::memory_order_relaxed) : 0;
        for (const auto& st : c->stripes) v += i < NFEC_DPATH_COUNT ? st->dec_paths[i].load(std::memory_order_relaxed) : 0;
        counts[i] = v;
    }
    return NFEC_DPATH_COUNT;
}

int nfec_codec_tail_batches(const nfec_codec* c, uint64_t* counts, uint32_t n)
{
    if (!c || (!counts && n)) return fail(NFEC_EINVAL, "null argument");
    for (uint32_t i = 0; i < n; ++i) {
        uint64_t v = i < 2 ? c->tail_batches[i].load(std::memory_order_relaxed) : 0;
        for (const auto& st : c->stripes) v += i < 2 ? st->tail_batches[i].load(std::memory_order_relaxed) : 0;
        counts[i] = v;
    }
    return 2;
}

int nfec_codec_get_generator(const nfec_codec* c, void* host_out, size_t bytes)
{
    if (!c || !host_out) return fail(NFEC_EINVAL, "null argument");
    const size_t need = (size_t)c->m * c->k * c->sym;
    if (bytes < need) return fail(NFEC_EINVAL, "output buffer too small");
    for (size_t i = 0; i < (size_t)c->m * c->k; ++i) {
        if (c->sym == 2) static_cast<uint16_t*>(host_out)[i] = (uint16_t)c->gen[i];
        else static_cast<uint8_t*>(host_out)[i] = (uint8_t)c->gen[i];
    }
    return NFEC_OK;
}

int nfec_encode(nfec_codec* codec, const nfec_block_batch* batch, void* stream)
{
    int rc = check_batch(codec, batch);
    if (rc || batch->nblocks == 0) return rc;
    if (!(codec = stripe_for(codec, batch->blocks))) return fail(NFEC_EINVAL, "batch is not on a device of the codec");
    DeviceGuard g(codec->device);
    return encode_device(codec, batch, static_cast<hipStream_t>(stream));
}

int nfec_decode(nfec_codec* codec, const nfec_block_batch* batch, const uint16_t* erasure_locs,
                uint32_t erasure_stride, const uint16_t* erasure_counts, int32_t* status, void* stream)
{
    int rc = check_batch(codec, batch);
    if (rc || batch->nblocks == 0) return rc;
    if (erasure_stride == 0) return fail(NFEC_EINVAL, "erasure_stride must be > 0");
    if (!(codec = stripe_for(codec, batch->blocks))) return fail(NFEC_EINVAL, "batch is not on a device of the codec");
    DeviceGuard g(codec->device);
    return decode_device(codec, batch, erasure_locs, erasure_stride, erasure_counts, status,
                         static_cast<hipStream_t>(stream));
}

// ---- receiver assembly on the device (kernels_rx.hip) ----
// Arguments are checked before the codec's device is: a null array or a short mask is
// NFEC_EINVAL on any codec, a host-only codec answers NFEC_EDEVICE to well-formed calls.
static BatchView batch_view(const nfec_codec* c, const nfec_block_batch* batch)
{
    BatchView v;
    v.base = static_cast<uint8_t*>(batch->blocks);
    v.block_stride = batch->block_stride;
    v.seg_stride = batch->seg_stride;
    v.nblocks = batch->nblocks;
    v.num_data = batch->num_data;
    v.k = c->k;
    v.m = c->m;
    v.vec = c->vec;
    return v;
}

static int check_mask(const nfec_codec* c, const uint32_t* received, uint32_t mask_stride)
{
    if (!received) return fail(NFEC_EINVAL, "null received mask");
    if ((uint64_t)mask_stride * 32u < (uint64_t)c->k + c->m)
        return fail(NFEC_EINVAL, "mask_stride smaller than (k + m + 31) / 32");
    return NFEC_OK;
}

int nfec_rx_place(const nfec_codec* codec, const nfec_block_batch* batch, const nfec_rx_segments* seg,
                  uint32_t* received, uint32_t mask_stride, uint32_t* stats, void* stream)
{
    if (!codec || !batch || !seg) return fail(NFEC_EINVAL, "null codec, batch or segments");
    int rc = check_mask(codec, received, mask_stride);
    if (rc) return rc;
    if (seg->count && !seg->payloads) return fail(NFEC_EINVAL, "null segments->payloads");
    if (seg->count && !seg->offsets) return fail(NFEC_EINVAL, "null segments->offsets");
    if (seg->count && !seg->block_index) return fail(NFEC_EINVAL, "null segments->block_index");
    if (seg->count && !seg->symbol_id) return fail(NFEC_EINVAL, "null segments->symbol_id");
    if (seg->count && !seg->length) return fail(NFEC_EINVAL, "null segments->length");
    if ((rc = check_batch(codec, batch)) || batch->nblocks == 0 || seg->count == 0) return rc;
    // (the stripe is only read: its shape and its device)
    const nfec_codec* c = stripe_for(const_cast<nfec_codec*>(codec), batch->blocks);
    if (!c) return fail(NFEC_EINVAL, "batch is not on a device of the codec");
    DeviceGuard g(c->device);
    RxPlaceArgs a;
    a.batch = batch_view(c, batch);
    a.payloads = static_cast<const uint8_t*>(seg->payloads);
    a.offsets = seg->offsets;
    a.block_index = seg->block_index;
    a.symbol_id = seg->symbol_id;
    a.length = seg->length;
    a.count = seg->count;
    a.received = received;
    a.mask_stride = mask_stride;
    a.stats = stats;
    return launch_rx_place(a, static_cast<hipStream_t>(stream));
}

int nfec_rx_ingest(const nfec_codec* codec, const nfec_block_batch* batch, const nfec_rx_messages* msg, uint8_t fec_id,
                   uint8_t fec_m, uint32_t first_block_id, uint32_t* received, uint32_t mask_stride,
                   uint32_t* block_index_out, uint16_t* symbol_id_out, uint32_t* stats, void* stream)
{
    if (!codec || !batch || !msg) return fail(NFEC_EINVAL, "null codec, batch or messages");
    int rc = check_mask(codec, received, mask_stride);
    if (rc) return rc;
    if (msg->count && !msg->payloads) return fail(NFEC_EINVAL, "null messages->payloads");
    if (msg->count && !msg->offsets) return fail(NFEC_EINVAL, "null messages->offsets");
    if (msg->count && !msg->length) return fail(NFEC_EINVAL, "null messages->length");
    const uint32_t id_kind = payload_id_kind(fec_id, fec_m);
    if (id_kind == PAYLOAD_ID_NONE) return fail(NFEC_EINVAL, "bad fec_id / fec_m");
    if ((rc = check_batch(codec, batch)) || batch->nblocks == 0 || msg->count == 0) return rc;
    // (the stripe is only read: its shape and its device)
    const nfec_codec* c = stripe_for(const_cast<nfec_codec*>(codec), batch->blocks);
    if (!c) return fail(NFEC_EINVAL, "batch is not on a device of the codec");
    DeviceGuard g(c->device);
    RxIngestArgs a;
    a.batch = batch_view(c, batch);
    a.payloads = static_cast<const uint8_t*>(msg->payloads);
    a.payload_bytes = msg->payload_bytes;
    a.offsets = msg->offsets;
    a.length = msg->length;
    a.count = msg->count;
    a.count_dev = msg->count_dev;
    a.id_kind = id_kind;
    a.first_block_id = first_block_id;
    a.received = received;
    a.mask_stride = mask_stride;
    a.block_index_out = block_index_out;
    a.symbol_id_out = symbol_id_out;
    a.stats = stats;
    return launch_rx_ingest(a, static_cast<hipStream_t>(stream));
}

int nfec_rx_erasures(const nfec_codec* codec, const uint32_t* received, uint32_t mask_stride, const uint16_t* num_data,
                     uint32_t nblocks, uint16_t* erasure_locs, uint32_t erasure_stride, uint16_t* erasure_counts,
                     void* stream)
{
    if (!codec) return fail(NFEC_EINVAL, "null codec");
    int rc = check_mask(codec, received, mask_stride);
    if (rc) return rc;
    if (!erasure_locs && erasure_stride) return fail(NFEC_EINVAL, "null erasure_locs");
    if (!erasure_counts) return fail(NFEC_EINVAL, "null erasure_counts");
    if (primary(codec)->host_only) return host_only_fail();
    if (nblocks == 0) return NFEC_OK;
    const nfec_codec* c = stripe_for(const_cast<nfec_codec*>(codec), received);
    if (!c) return fail(NFEC_EINVAL, "received mask is not on a device of the codec");
    DeviceGuard g(c->device);
    RxErasureArgs a;
    a.received = received;
    a.mask_stride = mask_stride;
    a.num_data = num_data;
    a.k = c->k;
    a.m = c->m;
    a.nblocks = nblocks;
    a.locs = erasure_locs;
    a.stride = erasure_stride;
    a.counts = erasure_counts;
    return launch_rx_erasures(a, static_cast<hipStream_t>(stream));
}

int nfec_decode_received(nfec_codec* codec, const nfec_block_batch* batch, const uint32_t* received,
                         uint32_t mask_stride, int32_t* status, void* stream)
{
    if (!codec || !batch) return fail(NFEC_EINVAL, "null codec or batch");
    int rc = check_mask(codec, received, mask_stride);
    if (rc) return rc;
    if ((rc = check_batch(codec, batch)) || batch->nblocks == 0) return rc;
    if (!(codec = stripe_for(codec, batch->blocks))) return fail(NFEC_EINVAL, "batch is not on a device of the codec");
    DeviceGuard g(codec->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the lists are decode workspace: held under the codec's mutex through the decode's own
    // launches, and reused by the next call in stream order, as the plan's buffers are
    std::lock_guard<std::mutex> lk(codec->mu);
    const uint32_t lstride = std::max(codec->m, 1u);
    if ((rc = codec->ws.rxlocs.reserve((size_t)batch->nblocks * lstride))) return rc;
    if ((rc = codec->ws.rxcounts.reserve(batch->nblocks))) return rc;
    RxErasureArgs a;
    a.received = received;
    a.mask_stride = mask_stride;
    a.num_data = batch->num_data;
    a.k = codec->k;
    a.m = codec->m;
    a.nblocks = batch->nblocks;
    a.locs = codec->ws.rxlocs.p;
    a.stride = lstride;
    a.counts = codec->ws.rxcounts.p;
    if ((rc = launch_rx_erasures(a, s))) return rc;
    return decode_device(codec, batch, codec->ws.rxlocs.p, lstride, codec->ws.rxcounts.p, status, s, true);
}

// ---- repair requests on the device (kernels_nack.hip) ----
int nfec_rx_repair_requests(const nfec_codec* codec, const uint32_t* received, uint32_t mask_stride,
                            const uint16_t* num_data, uint32_t nblocks, uint8_t fec_id, uint8_t fec_m, uint16_t object_id,
                            uint32_t first_block_id, uint32_t flags, uint32_t max_units, void* content, uint64_t capacity,
                            uint64_t* block_start, uint64_t* totals, void* stream)
{
    if (!codec) return fail(NFEC_EINVAL, "null codec");
    NackFormat f;
    int rc = nack_format(fec_id, fec_m, object_id, first_block_id, flags, max_units, &f);
    if (rc) return rc;
    if (nblocks && (rc = check_mask(codec, received, mask_stride))) return rc;
    if (!block_start || !totals) return fail(NFEC_EINVAL, "null block_start or totals");
    if (capacity && !content) return fail(NFEC_EINVAL, "null content");
    if (reinterpret_cast<uintptr_t>(content) & 3u) return fail(NFEC_EINVAL, "content is not 4-byte aligned");
    if (primary(codec)->host_only) return host_only_fail();
    const nfec_codec* c = stripe_for(const_cast<nfec_codec*>(codec), nblocks ? (const void*)received : block_start);
    if (!c) return fail(NFEC_EINVAL, "received mask is not on a device of the codec");
    DeviceGuard g(c->device);
    NackArgs a;
    a.received = received;
    a.mask_stride = mask_stride;
    a.num_data = num_data;
    a.k = c->k;
    a.m = c->m;
    a.nblocks = nblocks;
    a.id_kind = f.id_kind;
    a.item_len = f.item_len;
    a.fec_id = f.fec_id;
    a.object_id = f.object_id;
    a.first_block_id = f.first_block_id;
    a.info = f.info;
    a.max_units = f.max_units;
    a.content = static_cast<uint8_t*>(content);
    a.capacity = capacity;
    a.rows = block_start;
    a.totals = totals;
    return launch_nack(a, static_cast<hipStream_t>(stream));
}

// ---- sender repair state on the device (kernels_txrepair.hip) ----
static TxRepairState repair_state_view(const nfec_tx_repair_state* state)
{
    TxRepairState v;
    v.repair = state->repair, v.parity = state->parity, v.block_repair = state->block_repair, v.object = state->object;
    return v;
}

uint64_t nfec_tx_nack_workspace_bytes(uint32_t unit_capacity, uint32_t count, uint32_t nblocks)
{
    return tx_nack_workspace_bytes(unit_capacity, nblocks);
}

int nfec_tx_handle_nacks(const nfec_codec* codec, const nfec_rx_messages* nacks, uint8_t fec_id, uint8_t fec_m,
                         uint16_t object_id, uint32_t first_block_id, const uint16_t* num_data, uint32_t nblocks,
                         uint32_t mask_stride, uint32_t extra_parity, const nfec_tx_repair_state* state,
                         uint32_t unit_capacity, void* workspace, uint64_t workspace_bytes, uint64_t* totals, void* stream)
{
    if (!codec) return fail(NFEC_EINVAL, "null codec");
    uint32_t id_kind = 0;
    int rc = tx_nack_check(nacks, fec_id, fec_m, extra_parity, totals, &id_kind);
    if (rc || (rc = tx_repair_check(codec->k, codec->m, nblocks, mask_stride, state, "tx_handle_nacks"))) return rc;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u))
        return fail(NFEC_EINVAL, "tx_handle_nacks: workspace is null or not 16-byte aligned");
    if (workspace_bytes < tx_nack_workspace_bytes(unit_capacity, nblocks))
        return fail(NFEC_EINVAL, "tx_handle_nacks: workspace smaller than nfec_tx_nack_workspace_bytes");
    if (primary(codec)->host_only) return host_only_fail();
    const nfec_codec* c = stripe_for(const_cast<nfec_codec*>(codec), nblocks ? (const void*)state->repair : totals);
    if (!c) return fail(NFEC_EINVAL, "repair state is not on a device of the codec");
    DeviceGuard g(c->device);
    TxNackArgs a;
    a.payloads = static_cast<const uint8_t*>(nacks->payloads);
    a.payload_bytes = nacks->payload_bytes;
    a.offsets = nacks->offsets;
    a.length = nacks->length;
    a.count = nacks->count;
    a.count_dev = nacks->count_dev;
    a.id_kind = id_kind;
    a.fec_id = fec_id;
    a.object_id = object_id;
    a.first_block_id = first_block_id;
    a.num_data = num_data;
    a.k = c->k;
    a.m = c->m;
    a.nblocks = nblocks;
    a.mask_stride = mask_stride;
    a.extra_parity = extra_parity;
    a.state = repair_state_view(state);
    a.unit_capacity = unit_capacity;
    a.workspace = static_cast<uint8_t*>(workspace);
    a.totals = totals;
    return launch_tx_handle_nacks(a, static_cast<hipStream_t>(stream));
}

static int tx_activate_args(const nfec_codec* codec, const uint16_t* num_data, uint32_t nblocks, uint32_t auto_parity,
                            const uint32_t* pending, uint32_t mask_stride, const nfec_tx_repair_state* state,
                            const void* anchor, const char* what, TxActivateArgs* a, int* device)
{
    if (!codec) return fail(NFEC_EINVAL, "null codec");
    int rc = tx_repair_check(codec->k, codec->m, nblocks, mask_stride, state, what);
    if (rc) return rc;
    if (nblocks && !pending) return fail(NFEC_EINVAL, std::string(what) + ": null pending mask");
    if (auto_parity > codec->m) return fail(NFEC_EINVAL, std::string(what) + ": auto_parity above m");
    if (primary(codec)->host_only) return host_only_fail();
    if (nblocks == 0 && !anchor) return NFEC_OK;  // (nothing to launch, nothing to place on a device)
    const nfec_codec* c = stripe_for(const_cast<nfec_codec*>(codec), nblocks ? (const void*)pending : anchor);
    if (!c) return fail(NFEC_EINVAL, "pending mask is not on a device of the codec");
    a->num_data = num_data;
    a->k = c->k;
    a->m = c->m;
    a->nblocks = nblocks;
    a->auto_parity = auto_parity;
    a->pending = const_cast<uint32_t*>(pending);
    a->mask_stride = mask_stride;
    a->state = repair_state_view(state);
    *device = c->device;
    return NFEC_OK;
}

int nfec_tx_activate_repairs(const nfec_codec* codec, const uint16_t* num_data, uint32_t nblocks, uint32_t auto_parity,
                             uint32_t* pending, uint32_t mask_stride, const nfec_tx_repair_state* state, uint64_t* totals,
                             void* stream)
{
    if (!totals) return fail(NFEC_EINVAL, "tx_activate_repairs: null totals");
    TxActivateArgs a;
    int device = 0;
    int rc = tx_activate_args(codec, num_data, nblocks, auto_parity, pending, mask_stride, state, totals, "tx_activate_repairs",
                              &a, &device);
    if (rc) return rc;
    DeviceGuard g(device);
    a.totals = totals;
    return launch_tx_activate_repairs(a, static_cast<hipStream_t>(stream));
}

int nfec_tx_end_blocks(const nfec_codec* codec, const uint16_t* num_data, uint32_t nblocks, const uint32_t* pending,
                       uint32_t mask_stride, const nfec_tx_repair_state* state, void* stream)
{
    TxActivateArgs a;
    int device = 0;
    int rc = tx_activate_args(codec, num_data, nblocks, 0, pending, mask_stride, state, nullptr, "tx_end_blocks", &a, &device);
    if (rc || nblocks == 0) return rc;
    DeviceGuard g(device);
    return launch_tx_end_blocks(a, static_cast<hipStream_t>(stream));
}

// ---- NACK suppression and repair advertisements on the device (kernels_suppress.hip, kernels_nack.hip) ----
static RxRepairState rx_repair_state_view(const nfec_rx_repair_state* state)
{
    RxRepairState v;
    v.repair = state->repair, v.block_repair = state->block_repair, v.object = state->object;
    return v;
}

int nfec_rx_handle_repair_content(const nfec_codec* codec, const nfec_rx_messages* messages, uint8_t fec_id, uint8_t fec_m,
                                  uint16_t object_id, uint32_t first_block_id, const uint32_t* received, uint32_t mask_stride,
                                  const uint16_t* num_data, uint32_t nblocks, const nfec_rx_repair_state* state, uint64_t* totals,
                                  void* stream)
{
    if (!codec) return fail(NFEC_EINVAL, "null codec");
    uint32_t id_kind = 0;
    int rc = rx_content_check(messages, fec_id, fec_m, &id_kind);
    if (rc || (rc = rx_repair_check(codec->k, codec->m, nblocks, mask_stride, received, state, totals, "rx_handle_repair_content")))
        return rc;
    if (primary(codec)->host_only) return host_only_fail();
    const nfec_codec* c = stripe_for(const_cast<nfec_codec*>(codec), nblocks ? (const void*)state->repair : totals);
    if (!c) return fail(NFEC_EINVAL, "suppression state is not on a device of the codec");
    DeviceGuard g(c->device);
    RxRepairContentArgs a;
    a.payloads = static_cast<const uint8_t*>(messages->payloads);
    a.payload_bytes = messages->payload_bytes;
    a.offsets = messages->offsets;
    a.length = messages->length;
    a.count = messages->count;
    a.count_dev = messages->count_dev;
    a.id_kind = id_kind;
    a.fec_id = fec_id;
    a.object_id = object_id;
    a.first_block_id = first_block_id;
    a.received = received;
    a.mask_stride = mask_stride;
    a.num_data = num_data;
    a.k = c->k;
    a.m = c->m;
    a.nblocks = nblocks;
    a.state = rx_repair_state_view(state);
    a.totals = totals;
    return launch_rx_repair_content(a, static_cast<hipStream_t>(stream));
}

int nfec_rx_repair_pending(const nfec_codec* codec, const uint32_t* received, uint32_t mask_stride, const uint16_t* num_data,
                           uint32_t nblocks, const nfec_rx_repair_state* state, uint32_t flags, uint32_t* pending_blocks,
                           uint64_t* totals, void* stream)
{
    if (!codec) return fail(NFEC_EINVAL, "null codec");
    int rc = rx_repair_check(codec->k, codec->m, nblocks, mask_stride, received, state, totals, "rx_repair_pending");
    if (rc) return rc;
    if (flags & ~(uint32_t)NFEC_NACK_INFO) return fail(NFEC_EINVAL, "rx_repair_pending: unknown flags");
    if (primary(codec)->host_only) return host_only_fail();
    const nfec_codec* c = stripe_for(const_cast<nfec_codec*>(codec), nblocks ? (const void*)received : totals);
    if (!c) return fail(NFEC_EINVAL, "received mask is not on a device of the codec");
    DeviceGuard g(c->device);
    RxRepairPendingArgs a;
    a.received = received;
    a.mask_stride = mask_stride;
    a.num_data = num_data;
    a.k = c->k;
    a.m = c->m;
    a.nblocks = nblocks;
    a.state = rx_repair_state_view(state);
    a.info_pending = flags & NFEC_NACK_INFO;
    a.pending_blocks = pending_blocks;
    a.totals = totals;
    return launch_rx_repair_pending(a, static_cast<hipStream_t>(stream));
}

int nfec_tx_repair_adv(const nfec_codec* codec, const nfec_tx_repair_state* state, uint32_t mask_stride, const uint16_t* num_data,
                       uint32_t nblocks, uint8_t fec_id, uint8_t fec_m, uint16_t object_id, uint32_t first_block_id,
                       uint32_t max_units, void* content, uint64_t capacity, uint64_t* block_start, uint64_t* totals, void* stream)
{
    if (!codec) return fail(NFEC_EINVAL, "null codec");
    NackFormat f;
    int rc = nack_format(fec_id, fec_m, object_id, first_block_id, 0, max_units, &f);
    if (rc) return rc;
    if ((uint64_t)mask_stride * 32u < (uint64_t)codec->k + codec->m)
        return fail(NFEC_EINVAL, "tx_repair_adv: mask_stride smaller than (k + m + 31) / 32");
    if (!block_start || !totals) return fail(NFEC_EINVAL, "null block_start or totals");
    if (capacity && !content) return fail(NFEC_EINVAL, "null content");
    if (reinterpret_cast<uintptr_t>(content) & 3u) return fail(NFEC_EINVAL, "content is not 4-byte aligned");
    if (!state || (nblocks && (!state->repair || !state->block_repair || !state->object)))
        return fail(NFEC_EINVAL, "tx_repair_adv: null state");
    if (primary(codec)->host_only) return host_only_fail();
    const nfec_codec* c = stripe_for(const_cast<nfec_codec*>(codec), nblocks ? (const void*)state->repair : block_start);
    if (!c) return fail(NFEC_EINVAL, "repair state is not on a device of the codec");
    DeviceGuard g(c->device);
    NackArgs a;
    a.received = state->repair;
    a.block_repair = state->block_repair;
    a.object = state->object;
    a.mask_stride = mask_stride;
    a.num_data = num_data;
    a.k = c->k;
    a.m = c->m;
    a.nblocks = nblocks;
    a.id_kind = f.id_kind;
    a.item_len = f.item_len;
    a.fec_id = f.fec_id;
    a.object_id = f.object_id;
    a.first_block_id = f.first_block_id;
    a.max_units = f.max_units;
    a.content = static_cast<uint8_t*>(content);
    a.capacity = capacity;
    a.rows = block_start;
    a.totals = totals;
    return launch_repair_adv(a, static_cast<hipStream_t>(stream));
}

// ---- sender assembly on the device (kernels_tx.hip) ----
// The argument-check order is the receiver entries': arguments first, then the codec's device.
int nfec_tx_list(const nfec_codec* codec, const uint32_t* pending, uint32_t mask_stride, const uint16_t* num_data,
                 uint32_t nblocks, const uint16_t* seg_length, uint32_t length_stride, uint32_t gap, uint64_t* offsets,
                 uint32_t* block_index, uint16_t* symbol_id, uint16_t* length, uint32_t capacity, uint64_t* block_start,
                 void* stream)
{
    if (!codec) return fail(NFEC_EINVAL, "null codec");
    if (nblocks) {
        if (!pending) return fail(NFEC_EINVAL, "null pending mask");
        int rc = check_mask(codec, pending, mask_stride);
        if (rc) return rc;
    }
    if (seg_length && length_stride < codec->k) return fail(NFEC_EINVAL, "length_stride < k");
    if (capacity && (!offsets || !block_index || !symbol_id || !length)) return fail(NFEC_EINVAL, "null output array");
    if (!block_start) return fail(NFEC_EINVAL, "null block_start");
    if (primary(codec)->host_only) return host_only_fail();
    const nfec_codec* c = stripe_for(const_cast<nfec_codec*>(codec), nblocks ? (const void*)pending : block_start);
    if (!c) return fail(NFEC_EINVAL, "pending mask is not on a device of the codec");
    DeviceGuard g(c->device);
    TxListArgs a;
    a.pending = pending;
    a.mask_stride = mask_stride;
    a.num_data = num_data;
    a.k = c->k;
    a.m = c->m;
    a.vec = c->vec;
    a.nblocks = nblocks;
    a.seg_length = seg_length;
    a.length_stride = length_stride;
    a.gap = gap;
    a.offsets = offsets;
    a.block_index = block_index;
    a.symbol_id = symbol_id;
    a.length = length;
    a.capacity = capacity;
    a.block_start = block_start;
    return launch_tx_list(a, static_cast<hipStream_t>(stream));
}

int nfec_tx_emit(const nfec_codec* codec, const nfec_block_batch* batch, const nfec_tx_segments* seg, uint8_t fec_id,
                 uint8_t fec_m, uint32_t first_block_id, uint32_t* pending, uint32_t mask_stride, uint32_t* stats,
                 void* stream)
{
    if (!codec || !batch || !seg) return fail(NFEC_EINVAL, "null codec, batch or segments");
    int rc = pending ? check_mask(codec, pending, mask_stride) : NFEC_OK;
    if (rc) return rc;
    if (seg->count && !seg->payloads) return fail(NFEC_EINVAL, "null segments->payloads");
    if (seg->count && !seg->offsets) return fail(NFEC_EINVAL, "null segments->offsets");
    if (seg->count && !seg->block_index) return fail(NFEC_EINVAL, "null segments->block_index");
    if (seg->count && !seg->symbol_id) return fail(NFEC_EINVAL, "null segments->symbol_id");
    if (seg->count && !seg->length) return fail(NFEC_EINVAL, "null segments->length");
    // fec_id 0: no ID in front of the payloads
    const uint32_t id_kind = fec_id ? payload_id_kind(fec_id, fec_m) : (uint32_t)PAYLOAD_ID_NONE;
    if (fec_id && id_kind == PAYLOAD_ID_NONE) return fail(NFEC_EINVAL, "bad fec_id / fec_m");
    if ((rc = check_batch(codec, batch)) || batch->nblocks == 0 || seg->count == 0) return rc;
    const nfec_codec* c = stripe_for(const_cast<nfec_codec*>(codec), batch->blocks);
    if (!c) return fail(NFEC_EINVAL, "batch is not on a device of the codec");
    DeviceGuard g(c->device);
    TxEmitArgs a;
    a.batch = batch_view(c, batch);
    a.payloads = static_cast<uint8_t*>(seg->payloads);
    a.payload_bytes = seg->payload_bytes;
    a.offsets = seg->offsets;
    a.block_index = seg->block_index;
    a.symbol_id = seg->symbol_id;
    a.length = seg->length;
    a.count = seg->count;
    a.count_dev = seg->count_dev;
    a.id_kind = id_kind;
    a.first_block_id = first_block_id;
    a.pending = pending;
    a.mask_stride = mask_stride;
    a.stats = stats;
    return launch_tx_emit(a, static_cast<hipStream_t>(stream));
}

// ---- NORM_DATA messages on the device (kernels_datamsg.hip) ----
int nfec_tx_emit_data(const nfec_codec* codec, const nfec_block_batch* batch, const nfec_tx_segments* seg,
                      const nfec_data_header* header, uint32_t first_block_id, uint32_t* pending, uint32_t mask_stride,
                      uint64_t* msg_offsets_out, uint16_t* msg_length_out, uint32_t* stats, void* stream)
{
    if (!codec || !batch || !seg) return fail(NFEC_EINVAL, "null codec, batch or segments");
    int rc = pending ? check_mask(codec, pending, mask_stride) : NFEC_OK;
    if (rc) return rc;
    if (seg->count && !seg->payloads) return fail(NFEC_EINVAL, "null segments->payloads");
    if (seg->count && !seg->offsets) return fail(NFEC_EINVAL, "null segments->offsets");
    if (seg->count && !seg->block_index) return fail(NFEC_EINVAL, "null segments->block_index");
    if (seg->count && !seg->symbol_id) return fail(NFEC_EINVAL, "null segments->symbol_id");
    if (seg->count && !seg->length) return fail(NFEC_EINVAL, "null segments->length");
    TxEmitDataArgs a;
    if ((rc = data_header_fixed_from(header, a.header))) return rc;
    if ((rc = check_batch(codec, batch)) || batch->nblocks == 0 || seg->count == 0) return rc;
    const nfec_codec* c = stripe_for(const_cast<nfec_codec*>(codec), batch->blocks);
    if (!c) return fail(NFEC_EINVAL, "batch is not on a device of the codec");
    DeviceGuard g(c->device);
    a.tx.batch = batch_view(c, batch);
    a.tx.payloads = static_cast<uint8_t*>(seg->payloads);
    a.tx.payload_bytes = seg->payload_bytes;
    a.tx.offsets = seg->offsets;
    a.tx.block_index = seg->block_index;
    a.tx.symbol_id = seg->symbol_id;
    a.tx.length = seg->length;
    a.tx.count = seg->count;
    a.tx.count_dev = seg->count_dev;
    a.tx.id_kind = a.header.id_kind;
    a.tx.first_block_id = first_block_id;
    a.tx.pending = pending;
    a.tx.mask_stride = mask_stride;
    a.tx.stats = stats;
    a.msg_offsets_out = msg_offsets_out;
    a.msg_length_out = msg_length_out;
    return launch_tx_emit_data(a, static_cast<hipStream_t>(stream));
}

int nfec_rx_ingest_data(const nfec_codec* codec, const nfec_block_batch* batch, const nfec_rx_messages* msg,
                        const nfec_data_filter* filter, uint32_t first_block_id, uint32_t* received,
                        uint32_t mask_stride, uint8_t* class_out, uint16_t* sequence_out, uint32_t* block_index_out,
                        uint16_t* symbol_id_out, uint32_t* stats, uint64_t* totals, void* stream)
{
    if (!codec || !batch || !msg) return fail(NFEC_EINVAL, "null codec, batch or datagrams");
    int rc = check_mask(codec, received, mask_stride);
    if (rc) return rc;
    if (msg->count && !msg->payloads) return fail(NFEC_EINVAL, "null datagrams->payloads");
    if (msg->count && !msg->offsets) return fail(NFEC_EINVAL, "null datagrams->offsets");
    if (msg->count && !msg->length) return fail(NFEC_EINVAL, "null datagrams->length");
    RxIngestDataArgs a;
    if ((rc = data_filter_from(filter, a.filter))) return rc;
    if ((rc = check_batch(codec, batch)) || batch->nblocks == 0 || msg->count == 0) return rc;
    // (the stripe is only read: its shape and its device)
    const nfec_codec* c = stripe_for(const_cast<nfec_codec*>(codec), batch->blocks);
    if (!c) return fail(NFEC_EINVAL, "batch is not on a device of the codec");
    DeviceGuard g(c->device);
    a.rx.batch = batch_view(c, batch);
    a.rx.payloads = static_cast<const uint8_t*>(msg->payloads);
    a.rx.payload_bytes = msg->payload_bytes;
    a.rx.offsets = msg->offsets;
    a.rx.length = msg->length;
    a.rx.count = msg->count;
    a.rx.count_dev = msg->count_dev;
    a.rx.id_kind = a.filter.id_kind;
    a.rx.first_block_id = first_block_id;
    a.rx.received = received;
    a.rx.mask_stride = mask_stride;
    a.rx.block_index_out = block_index_out;
    a.rx.symbol_id_out = symbol_id_out;
    a.rx.stats = stats;
    a.class_out = class_out;
    a.sequence_out = sequence_out;
    a.totals = totals;
    return launch_rx_ingest_data(a, static_cast<hipStream_t>(stream));
}

// ---- NORM_NACK and NORM_CMD(REPAIR_ADV) messages on the device (kernels_ctlmsg.hip) ----
uint64_t nfec_nack_fragment_workspace_bytes(uint64_t content_capacity, uint32_t nblocks)
{
    return nack_fragment_workspace(content_capacity, nblocks);
}

int nfec_nack_fragment(const nfec_codec* codec, const void* content, uint64_t content_capacity,
                       const uint64_t* content_bytes_dev, const uint64_t* block_start, uint32_t nblocks, uint8_t fec_id,
                       uint32_t segment_size, const nfec_nack_header* header, void* wire, uint64_t wire_bytes, uint32_t pitch,
                       uint64_t* msg_offsets_out, uint16_t* msg_length_out, uint32_t capacity, uint64_t* totals,
                       void* workspace, uint64_t workspace_bytes, void* stream)
{
    if (!codec) return fail(NFEC_EINVAL, "null codec");
    NackFragmentArgs a;
    int rc = nack_header_fixed_from(header, a.header);
    if (rc || (rc = cut_params_from(fec_id, segment_size, a.header.hdr_bytes, a.cut, "nack_fragment"))) return rc;
    if (!content || !content_bytes_dev || !totals) return fail(NFEC_EINVAL, "nack_fragment: null content, content_bytes_dev or totals");
    if (reinterpret_cast<uintptr_t>(content) & 3u) return fail(NFEC_EINVAL, "nack_fragment: content is not 4-byte aligned");
    if (content_capacity >> 32) return fail(NFEC_ERANGE, "nack_fragment: content_capacity of 2^32 or more");
    if (!block_start && nblocks) return fail(NFEC_EINVAL, "nack_fragment: null block_start with nblocks > 0");
    if ((pitch & 3u) || pitch < a.header.hdr_bytes + a.cut.S)
        return fail(NFEC_EINVAL, "nack_fragment: pitch is no multiple of 4 or below header + segment_size");
    if (capacity && (!wire || (reinterpret_cast<uintptr_t>(wire) & 3u)))
        return fail(NFEC_EINVAL, "nack_fragment: wire is null or not 4-byte aligned");
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u) ||
        workspace_bytes < nack_fragment_workspace(content_capacity, block_start ? nblocks : 0))
        return fail(NFEC_EINVAL, "nack_fragment: workspace is null, not 8-byte aligned or below nfec_nack_fragment_workspace_bytes");
    if (primary(codec)->host_only) return host_only_fail();
    const nfec_codec* c = stripe_for(const_cast<nfec_codec*>(codec), content);
    if (!c) return fail(NFEC_EINVAL, "content is not on a device of the codec");
    DeviceGuard g(c->device);
    a.content = static_cast<const uint32_t*>(content);
    a.content_capacity = content_capacity;
    a.content_bytes_dev = content_bytes_dev;
    a.block_start = block_start;
    a.nblocks = block_start ? nblocks : 0;
    a.wire = static_cast<uint8_t*>(wire);
    a.pitch = pitch;
    a.msg_offsets_out = msg_offsets_out;
    a.msg_length_out = msg_length_out;
    a.capacity = (uint32_t)std::min<uint64_t>(capacity, wire_bytes / pitch);
    a.totals = totals;
    a.workspace = static_cast<uint8_t*>(workspace);
    return launch_nack_fragment(a, static_cast<hipStream_t>(stream));
}

int nfec_tx_repair_adv_message(const nfec_codec* codec, const void* content, uint64_t content_capacity,
                               const uint64_t* content_bytes_dev, uint8_t fec_id, uint32_t segment_size,
                               const nfec_adv_header* header, void* wire, uint64_t wire_bytes, uint16_t* msg_length_out,
                               uint64_t* totals, void* stream)
{
    if (!codec) return fail(NFEC_EINVAL, "null codec");
    AdvMessageArgs a;
    int rc = adv_header_fixed_from(header, a.header);
    if (rc || (rc = cut_params_from(fec_id, segment_size, a.header.hdr_bytes, a.cut, "tx_repair_adv_message"))) return rc;
    if (!content || !content_bytes_dev || !totals || !msg_length_out)
        return fail(NFEC_EINVAL, "tx_repair_adv_message: null content, content_bytes_dev, msg_length_out or totals");
    if (reinterpret_cast<uintptr_t>(content) & 3u) return fail(NFEC_EINVAL, "tx_repair_adv_message: content is not 4-byte aligned");
    if (content_capacity >> 32) return fail(NFEC_ERANGE, "tx_repair_adv_message: content_capacity of 2^32 or more");
    if (!wire || (reinterpret_cast<uintptr_t>(wire) & 3u) || wire_bytes < (uint64_t)a.header.hdr_bytes + a.cut.S)
        return fail(NFEC_EINVAL, "tx_repair_adv_message: wire is null, not 4-byte aligned or below header + segment_size");
    if (primary(codec)->host_only) return host_only_fail();
    const nfec_codec* c = stripe_for(const_cast<nfec_codec*>(codec), content);
    if (!c) return fail(NFEC_EINVAL, "content is not on a device of the codec");
    DeviceGuard g(c->device);
    a.content = static_cast<const uint32_t*>(content);
    a.content_capacity = content_capacity;
    a.content_bytes_dev = content_bytes_dev;
    a.wire = static_cast<uint32_t*>(wire);
    a.msg_length_out = msg_length_out;
    a.totals = totals;
    return launch_adv_message(a, static_cast<hipStream_t>(stream));
}

int nfec_rx_ingest_control(const nfec_codec* codec, const nfec_rx_messages* msg, const nfec_ctl_filter* filter, uint8_t* class_out,
                           uint64_t* content_offset_out, uint16_t* content_length_out, uint32_t* source_id_out,
                           uint32_t* grtt_response_out, uint32_t* stats, void* stream)
{
    if (!codec || !msg) return fail(NFEC_EINVAL, "null codec or datagrams");
    CtlIngestArgs a;
    int rc = ctl_filter_from(filter, a.filter);
    if (rc) return rc;
    if (msg->count && (!msg->payloads || !msg->offsets || !msg->length)) return fail(NFEC_EINVAL, "null datagrams array");
    if (msg->count && (!content_offset_out || !content_length_out))
        return fail(NFEC_EINVAL, "rx_ingest_control: null content_offset_out or content_length_out");
    if (primary(codec)->host_only) return host_only_fail();
    if (msg->count == 0) return NFEC_OK;
    const nfec_codec* c = stripe_for(const_cast<nfec_codec*>(codec), msg->payloads);
    if (!c) return fail(NFEC_EINVAL, "wire buffer is not on a device of the codec");
    DeviceGuard g(c->device);
    a.payloads = static_cast<const uint8_t*>(msg->payloads);
    a.payload_bytes = msg->payload_bytes;
    a.offsets = msg->offsets;
    a.length = msg->length;
    a.count = msg->count;
    a.count_dev = msg->count_dev;
    a.class_out = class_out;
    a.content_offset_out = content_offset_out;
    a.content_length_out = content_length_out;
    a.source_id_out = source_id_out;
    a.grtt_response_out = grtt_response_out;
    a.stats = stats;
    return launch_ctl_ingest(a, static_cast<hipStream_t>(stream));
}

// ---- object segmentation on the device (kernels_obj.hip) ----
// Arguments first, then the codec's device, as above.  The layout is taken only as
// nfec_object_layout_for makes it: the kernels index the object and the batch by its fields, so a
// layout that is not one cannot make a call read or write outside either.
static int check_object_call(const nfec_codec* codec, const nfec_object_layout* layout, const void* object,
                             const nfec_block_batch* batch, uint32_t first_block)
{
    if (!codec || !layout || !batch) return fail(NFEC_EINVAL, "null codec, layout or batch");
    if (!object) return fail(NFEC_EINVAL, "null object");
    nfec_object_layout want;
    if (nfec_object_layout_for(layout->object_size, layout->segment_size, layout->num_data, &want) != NFEC_OK ||
        want.num_segments != layout->num_segments || want.num_blocks != layout->num_blocks ||
        want.large_block_size != layout->large_block_size || want.large_block_count != layout->large_block_count ||
        want.small_block_size != layout->small_block_size || want.small_block_count != layout->small_block_count ||
        want.final_block_id != layout->final_block_id || want.final_segment_size != layout->final_segment_size)
        return fail(NFEC_EINVAL, "layout is not one nfec_object_layout_for made");
    if (layout->num_data != codec->k) return fail(NFEC_EINVAL, "layout->num_data != k");
    if (layout->segment_size > codec->vec) return fail(NFEC_EINVAL, "segment_size > vector_size");
    if ((uint64_t)first_block + batch->nblocks > layout->num_blocks)
        return fail(NFEC_EINVAL, "first_block + nblocks > num_blocks");
    return NFEC_OK;
}

// the stripe that holds the batch; an object in another device's memory is refused where HIP can tell
static const nfec_codec* object_stripe(const nfec_codec* codec, const void* object, const nfec_block_batch* batch)
{
    const nfec_codec* c = stripe_for(const_cast<nfec_codec*>(codec), batch->blocks);
    if (!c) {
        fail(NFEC_EINVAL, "batch is not on a device of the codec");
        return nullptr;
    }
    hipPointerAttribute_t ao, ab;
    std::memset(&ao, 0, sizeof(ao));
    std::memset(&ab, 0, sizeof(ab));
    if (hipPointerGetAttributes(&ao, object) != hipSuccess || hipPointerGetAttributes(&ab, batch->blocks) != hipSuccess) {
        (void)hipGetLastError();
        fail(NFEC_EINVAL, "object is not memory HIP knows");
        return nullptr;
    }
    if (ao.type == hipMemoryTypeDevice && ab.type == hipMemoryTypeDevice && ao.device != ab.device) {
        fail(NFEC_EINVAL, "object and batch are on different devices");
        return nullptr;
    }
    return c;
}

static void object_args(ObjArgs& a, const nfec_codec* c, const nfec_object_layout* layout, const void* object,
                        uint64_t object_bytes, uint32_t first_block, const nfec_block_batch* batch)
{
    a.batch = batch_view(c, batch);
    a.object = static_cast<uint8_t*>(const_cast<void*>(object));
    a.object_bytes = object_bytes;
    a.first_block = first_block;
    a.lay = *layout;
}

int nfec_object_read(const nfec_codec* codec, const nfec_object_layout* layout, const void* object, uint64_t object_bytes,
                     uint32_t first_block, const nfec_block_batch* batch, uint16_t* num_data_out,
                     uint16_t* seg_length_out, uint32_t length_stride, void* stream)
{
    int rc = check_object_call(codec, layout, object, batch, first_block);
    if (rc) return rc;
    if (object_bytes < layout->object_size) return fail(NFEC_EINVAL, "object_bytes < object_size");
    if (seg_length_out && length_stride < codec->k) return fail(NFEC_EINVAL, "length_stride < k");
    if ((rc = check_batch(codec, batch)) || batch->nblocks == 0) return rc;
    const nfec_codec* c = object_stripe(codec, object, batch);
    if (!c) return NFEC_EINVAL;
    DeviceGuard g(c->device);
    ObjArgs a;
    object_args(a, c, layout, object, object_bytes, first_block, batch);
    a.num_data_out = num_data_out;
    a.seg_length_out = seg_length_out;
    a.length_stride = length_stride;
    return launch_obj_read(a, static_cast<hipStream_t>(stream));
}

int nfec_object_write(const nfec_codec* codec, const nfec_object_layout* layout, void* object, uint64_t object_bytes,
                      uint32_t first_block, const nfec_block_batch* batch, const uint32_t* received,
                      uint32_t mask_stride, const int32_t* status, uint32_t* stats, void* stream)
{
    int rc = check_object_call(codec, layout, object, batch, first_block);
    if (rc) return rc;
    if (received && (rc = check_mask(codec, received, mask_stride))) return rc;
    if ((rc = check_batch(codec, batch)) || batch->nblocks == 0) return rc;
    const nfec_codec* c = object_stripe(codec, object, batch);
    if (!c) return NFEC_EINVAL;
    DeviceGuard g(c->device);
    ObjArgs a;
    object_args(a, c, layout, object, object_bytes, first_block, batch);
    a.received = received;
    a.mask_stride = mask_stride;
    a.status = status;
    a.stats = stats;
    return launch_obj_write(a, static_cast<hipStream_t>(stream));
}

// ---- stream objects on the device (kernels_stream.hip) ----
// Arguments first, then the codec's device, as above.
int nfec_stream_frame(const nfec_codec* codec, uint32_t segment_size, const uint32_t* write_len, const uint8_t* write_flags,
                      uint32_t n, nfec_stream_state state, nfec_stream_state* state_out, uint64_t* seg_start,
                      uint16_t* seg_len, uint16_t* seg_msg_start, uint32_t capacity, uint64_t* totals, void* workspace,
                      void* stream)
{
    if (!codec) return fail(NFEC_EINVAL, "null codec");
    if (!state_out || !totals || !workspace) return fail(NFEC_EINVAL, "stream_frame: null state_out, totals or workspace");
    if (n && (!write_len || !write_flags)) return fail(NFEC_EINVAL, "stream_frame: null write arrays");
    if (n == 0xffffffffu) return fail(NFEC_EINVAL, "stream_frame: more than 2^32 - 2 writes");
    if (capacity && (!seg_start || !seg_len || !seg_msg_start)) return fail(NFEC_EINVAL, "stream_frame: null output array");
    int rc = check_stream_frame(segment_size, &state);
    if (rc) return rc;
    if (primary(codec)->host_only) return host_only_fail();
    const nfec_codec* c = stripe_for(const_cast<nfec_codec*>(codec), totals);
    if (!c) return fail(NFEC_EINVAL, "totals is not on a device of the codec");
    DeviceGuard g(c->device);
    StreamFrameArgs a;
    a.S = segment_size;
    a.write_len = write_len;
    a.write_flags = write_flags;
    a.n = n;
    a.state = state;
    a.state_out = state_out;
    a.seg_start = seg_start;
    a.seg_len = seg_len;
    a.seg_msg_start = seg_msg_start;
    a.capacity = capacity;
    a.totals = totals;
    a.ws = static_cast<uint64_t*>(workspace);
    return launch_stream_frame(a, static_cast<hipStream_t>(stream));
}

static int check_stream_copy(const nfec_codec* codec, const nfec_block_batch* batch, uint32_t segment_size)
{
    if (!codec || !batch) return fail(NFEC_EINVAL, "null codec or batch");
    if (segment_size < 1 || (uint64_t)segment_size + 8u > codec->vec)
        return fail(NFEC_EINVAL, "segment_size outside [1, vector_size - 8]");
    return NFEC_OK;
}

int nfec_stream_pack(const nfec_codec* codec, const nfec_stream_segments* seg, uint32_t segment_size, uint64_t first_slot,
                     uint32_t write_offset, uint32_t flags, const nfec_block_batch* batch, uint16_t* num_data_out,
                     uint16_t* seg_length_out, uint32_t length_stride, uint32_t* stats, void* stream)
{
    if (!seg) return fail(NFEC_EINVAL, "null segments");
    int rc = check_stream_copy(codec, batch, segment_size);
    if (rc) return rc;
    if (flags & ~NFEC_STREAM_END) return fail(NFEC_EINVAL, "stream_pack: unknown flags");
    if (seg->count && (!seg->seg_start || !seg->seg_len || !seg->seg_msg_start))
        return fail(NFEC_EINVAL, "null segments->seg_start, seg_len or seg_msg_start");
    if (seg->count && !seg->bytes) return fail(NFEC_EINVAL, "null segments->bytes");
    if (seg_length_out && length_stride < codec->k) return fail(NFEC_EINVAL, "length_stride < k");
    if (first_slot > (1ull << 63)) return fail(NFEC_EINVAL, "first_slot above 2^63");
    const uint32_t end = flags & NFEC_STREAM_END ? 1u : 0u;
    if ((rc = check_batch(codec, batch)) || batch->nblocks == 0 || (seg->count == 0 && !end)) return rc;
    const nfec_codec* c = seg->bytes ? object_stripe(codec, seg->bytes, batch)
                                     : stripe_for(const_cast<nfec_codec*>(codec), batch->blocks);
    if (!c) return seg->bytes ? NFEC_EINVAL : fail(NFEC_EINVAL, "batch is not on a device of the codec");
    DeviceGuard g(c->device);
    StreamPackArgs a;
    a.batch = batch_view(c, batch);
    a.bytes = static_cast<const uint8_t*>(seg->bytes);
    a.stream_bytes = seg->stream_bytes;
    a.seg_start = seg->seg_start;
    a.seg_len = seg->seg_len;
    a.seg_msg_start = seg->seg_msg_start;
    a.count = seg->count;
    a.count_dev = seg->count ? seg->count_dev : nullptr;
    a.S = segment_size;
    a.first_slot = first_slot;
    a.write_offset = write_offset;
    a.end = end;
    a.num_data_out = num_data_out;
    a.seg_length_out = seg_length_out;
    a.length_stride = length_stride;
    a.stats = stats;
    return launch_stream_pack(a, static_cast<hipStream_t>(stream));
}

int nfec_stream_unpack(const nfec_codec* codec, const nfec_block_batch* batch, const uint32_t* received,
                       uint32_t mask_stride, const int32_t* status, void* window, uint64_t window_bytes,
                       uint32_t base_offset, uint32_t segment_size, uint32_t* offset_out, uint16_t* len_out,
                       uint16_t* msg_start_out, uint32_t out_stride, uint32_t* stats, void* stream)
{
    int rc = check_stream_copy(codec, batch, segment_size);
    if (rc) return rc;
    if (!window) return fail(NFEC_EINVAL, "null window");
    if (received && (rc = check_mask(codec, received, mask_stride))) return rc;
    if ((offset_out || len_out || msg_start_out) && out_stride < codec->k) return fail(NFEC_EINVAL, "out_stride < k");
    if ((rc = check_batch(codec, batch)) || batch->nblocks == 0) return rc;
    const nfec_codec* c = object_stripe(codec, window, batch);
    if (!c) return NFEC_EINVAL;
    DeviceGuard g(c->device);
    StreamUnpackArgs a;
    a.batch = batch_view(c, batch);
    a.received = received;
    a.mask_stride = mask_stride;
    a.status = status;
    a.window = static_cast<uint8_t*>(window);
    a.window_bytes = window_bytes;
    a.base_offset = base_offset;
    a.S = segment_size;
    a.offset_out = offset_out;
    a.len_out = len_out;
    a.msg_start_out = msg_start_out;
    a.out_stride = out_stride;
    a.stats = stats;
    return launch_stream_unpack(a, static_cast<hipStream_t>(stream));
}

// ---- per-call NORM semantics (synchronous, host vectors) ----
// One call = gather the caller's vectors into the codec's pinned staging (host memcpy), one
// H2D copy, the kernels, one D2H copy of what the call writes, one synchronize, scatter.  The
// staging layout (device and pinned alike):
//   [0, 8)                 decode status (int32)
//   [8, 8 + meta)          decode erasure list (m uint16), count, numData
//   [data0, ...)           slots of round_up(vec, 8) bytes
// Per call this is latency-bound ("per-call drop-in"): NORM's block-at-once
// sites should use the batch calls instead.
namespace {

struct PerCall {
    uint8_t* dev;
    uint8_t* pin;
    uint32_t stride, data0;
};

int per_call_stage(nfec_codec* c, uint32_t nslots, PerCall& pc)
{
    pc.stride = round_up(c->vec, 8);
    pc.data0 = 8 + round_up((c->m + 2) * 2, 8);
    const size_t bytes = pc.data0 + (size_t)nslots * pc.stride;
    int rc = c->s_block.reserve(bytes);
    if (rc) return rc;
    if (c->s_pin_bytes < bytes) {
        if (c->s_pin) (void)hipHostFree(c->s_pin);
        c->s_pin = nullptr;
        c->s_pin_bytes = 0;
        if (hipHostMalloc(reinterpret_cast<void**>(&c->s_pin), bytes, hipHostMallocDefault) != hipSuccess)
            return fail(NFEC_ENOMEM, "per-call pinned staging allocation failed");
        c->s_pin_bytes = bytes;
    }
    if (!c->s_stream && hipStreamCreateWithFlags(&c->s_stream, hipStreamNonBlocking) != hipSuccess)
        return fail(NFEC_ENOMEM, "per-call stream creation failed");
    pc.dev = c->s_block.p;
    pc.pin = c->s_pin;
    return NFEC_OK;
}

}  // namespace

int nfec_encode_segment(nfec_codec* c, uint32_t segment_id, const void* data, void* const* parity)
{
    if (!c || !data || !parity) return fail(NFEC_EINVAL, "null argument");
    c = primary(c);
    if (c->host_only) return host_only_fail();
    if (segment_id >= c->k) return fail(NFEC_EINVAL, "segmentId >= numData");
    for (uint32_t i = 0; i < c->m; ++i)
        if (!parity[i]) return fail(NFEC_EINVAL, "null parity vector");
    DeviceGuard g(c->device);
    std::lock_guard<std::mutex> lk(c->mu);
    // slots: data, P0..P(m-1), and for MDP the new P(0..m-1) after them
    const uint32_t nslots = c->kind == NFEC_MDP ? 2 * c->m + 1 : c->m + 1;
    PerCall pc;
    int rc = per_call_stage(c, nslots, pc);
    if (rc) return rc;
    const hipStream_t st = c->s_stream;
    uint8_t* hp = pc.pin + pc.data0;
    // (measured: a kernel reading and writing the pinned staging directly, with no copies, is
    // slower per call -- 140 against 82 us for RS8(64,32): its loads cross PCIe one by one)
    uint8_t* d = pc.dev + pc.data0;
    std::memcpy(hp, data, c->vec);
    for (uint32_t i = 0; i < c->m; ++i) std::memcpy(hp + (size_t)(1 + i) * pc.stride, parity[i], c->vec);
    NFEC_HIP(hipMemcpyAsync(d, hp, (size_t)(c->m + 1) * pc.stride, hipMemcpyHostToDevice, st));
    uint32_t out_first = 1;
    if (c->kind == NFEC_RS8 || c->kind == NFEC_MDP) {
        Gf8MatmulArgs a;
        a.in_base = d;
        a.in_seg_stride = pc.stride;
        a.out_base = d;
        a.out_seg_stride = pc.stride;
        a.out_slot_mode = OUT_SLOT_AFTER_INPUT;
        a.rows_const = c->m;
        a.coef_col_stride = c->cs;
        a.vtab = c->d_vtab.p;
        a.nblocks = 1;
        a.vec_bytes = c->vec;
        if (c->kind == NFEC_RS8) {
            a.cols_const = 1;  // data in slot 0, column segment_id of the generator
            a.coef = c->d_coef.p + (size_t)segment_id * c->cs;
            a.accumulate = 1;  // parity[i] ^= G[k+i][segment_id] * data  (normEncoderRS8.cpp:473-483)
        } else {
            a.cols_const = c->m + 1;  // [d, P0..P(m-1)] -> new P in slots m+1..2m
            a.coef = c->d_mdp_step.p;
            out_first = c->m + 1;
        }
        if ((rc = launch_gf8_matmul(a, false, st))) return rc;
    } else {
        // the tower kernel over one column: the generator column segment_id is its own block
        // of the codec's table; parity slots 1..m, accumulated (normEncoderRS16.cpp:472-482).
        // A layout it does not take (its 2^31 offset bounds) goes to the exp-table kernel.
        Gf16T3Args t;
        t.base = d;
        t.block_stride = (uint64_t)(c->m + 1) * pc.stride;
        t.seg_stride = pc.stride;
        t.nblocks = 1;
        t.k = 1;
        t.m = c->m;
        t.vec_bytes = c->vec & ~1u;
        t.tw = c->tw ? c->d_twoff.p + (size_t)segment_id * 4u * c->m : nullptr;
        t.accumulate = 1;
        rc = c->tw && rs16_tw_full_covers(t) ? launch_rs16_tw_full(t, st) : NFEC_ENOTSUP;
        if (rc != NFEC_ENOTSUP && rc) return rc;
        if (rc == NFEC_ENOTSUP) {
            Gf16MatmulArgs a;
            a.in_base = d;
            a.in_seg_stride = pc.stride;
            a.cols_const = 1;
            a.out_base = d;
            a.out_seg_stride = pc.stride;
            a.out_slot_mode = OUT_SLOT_AFTER_INPUT;
            a.rows_const = c->m;
            a.coef = reinterpret_cast<const uint16_t*>(c->d_coef.p) + (size_t)segment_id * c->cs;
            a.coef_col_stride = c->cs;
            a.exp_tab = reinterpret_cast<const uint16_t*>(c->d_exp.p);
            a.log_tab = c->d_log.p;
            a.nblocks = 1;
            a.vec_bytes = c->vec & ~1u;
            a.accumulate = 1;
            if ((rc = launch_gf16_matmul(a, st))) return rc;
        }
    }
    const size_t off = (size_t)out_first * pc.stride;
    NFEC_HIP(hipMemcpyAsync(hp + off, d + off, (size_t)c->m * pc.stride, hipMemcpyDeviceToHost, st));
    NFEC_HIP(hipStreamSynchronize(st));
    // RS16 never writes an odd last byte: it came back unchanged from the upload
    for (uint32_t i = 0; i < c->m; ++i) std::memcpy(parity[i], hp + off + (size_t)i * pc.stride, c->vec);
    return NFEC_OK;
}

int nfec_encode_segment_host(nfec_codec* c, uint32_t segment_id, const void* data, void* const* parity)
{
    if (!c || !data || !parity) return fail(NFEC_EINVAL, "null argument");
    c = primary(c);  // a multi-device codec: the first stripe holds the host tables (mdp_g)
    if (segment_id >= c->k) return fail(NFEC_EINVAL, "segmentId >= numData");
    for (uint32_t i = 0; i < c->m; ++i)
        if (!parity[i]) return fail(NFEC_EINVAL, "null parity vector");
    const uint8_t* d = static_cast<const uint8_t*>(data);
    const int isa = host_gf8_isa();
    if (c->kind == NFEC_RS16) {
        // vec / 2 native-endian symbols; an odd last byte is never touched (normEncoderRS16.cpp:479)
        host_gf16_addmul_rows(reinterpret_cast<uint16_t* const*>(parity), static_cast<const uint16_t*>(data),
                              c->gen.data() + segment_id, c->k, c->m, c->vec / 2, isa);
        return NFEC_OK;
    }
    if (c->kind == NFEC_MDP) {
        // the reference's LFSR step: s = data ^ P0 (its scratch copy of P0), then the shift
        host_mdp_step(reinterpret_cast<uint8_t* const*>(parity), d, c->mdp_g.data(), c->m, c->vec, isa);
        return NFEC_OK;
    }
    host_gf8_addmul_rows(reinterpret_cast<uint8_t* const*>(parity), d, c->gen.data() + segment_id, c->k, c->m, c->vec,
                         isa);
    return NFEC_OK;
}

// The host repair's products: dst[r] (^)= sum_j coef[r][j] * srcs[j] over nelem bytes (GF(2^8))
// or symbols (GF(2^16)), row dot products over pieces of the vectors, so a piece of every column
// stays in cache while all rows take it; a repair of more than 8 MiB of products splits the
// vectors over host threads (disjoint element ranges, no sharing).
static int host_rows_apply(bool wide, void* const* dst, uint32_t nrows, const void* const* srcs, uint32_t ncol,
                           const uint16_t* coef, size_t nelem, bool acc)
{
    const int isa = host_gf8_isa();
    const uint64_t work = (uint64_t)nrows * ncol * nelem * (wide ? 2 : 1);
    const size_t piece = wide ? 1024 : 2048;
    auto run = [&](size_t e0, size_t e1) {
        for (size_t c0 = e0; c0 < e1; c0 += piece) {
            const size_t len = std::min(piece, e1 - c0);
            for (uint32_t r = 0; r < nrows; ++r) {
                if (!dst[r]) continue;
                if (wide)
                    host_gf16_dot(static_cast<uint16_t*>(dst[r]) + c0, reinterpret_cast<const uint16_t* const*>(srcs), c0,
                                  coef + (size_t)r * ncol, ncol, len, acc, isa);
                else
                    host_gf8_dot(static_cast<uint8_t*>(dst[r]) + c0, reinterpret_cast<const uint8_t* const*>(srcs), c0,
                                 coef + (size_t)r * ncol, ncol, len, acc, isa);
            }
        }
    };
    const unsigned nt = work > (8ull << 20)
                            ? (unsigned)std::min<uint64_t>(std::min<uint64_t>(host_pool_size(), work >> 22), nelem / 256)
                            : 1u;
    if (nt <= 1) {
        run(0, nelem);
        return NFEC_OK;
    }
    // ranges in multiples of 128 elements, on the process's host pool
    const size_t per = ((nelem + nt - 1) / nt + 127) & ~(size_t)127;
    return host_parallel_for(nt, [&](unsigned t) {
        const size_t e0 = std::min(nelem, t * per), e1 = std::min(nelem, e0 + per);
        if (e0 < e1) run(e0, e1);
    });
}

// MDP one-block repair on the host: the closed-form Forney map of mdp_plan_kernel
// (kernels_plan.hip; tests/test_mdp_algebra.py), C[r][v] = [Dinv_r beta_r^m] [gamma_v^(m+1)
// Lambda(1 / gamma_v)] / (gamma_v beta_r + 1) over the surviving slots v, written over the erased
// source (the reference's syndrome decode, normEncoderMDP.cpp:333-430, reads erased source as
// zeros and missing parity as absent).  The list is already validated and es > 0.
static int mdp_decode_host(const nfec_codec* c, void* const* vectors, uint32_t nd, uint32_t ec,
                            const uint32_t* locs, uint32_t es)
{
    const Field& f = gf8();
    const uint32_t m = c->m, nvecs = nd + m, deg = 2 * m;
    auto mul = [&](uint32_t x, uint32_t y) -> uint32_t { return (x && y) ? f.exp[f.log[x] + f.log[y]] : 0u; };
    // erasure locator lambda(x) = prod_i (1 + X_i x), X_i = alpha^(nvecs-1-loc_i)
    std::vector<uint32_t> lam(deg, 0);
    lam[0] = 1;
    for (uint32_t i = 0; i < ec; ++i) {
        const uint32_t X = f.exp[nvecs - 1 - locs[i]];
        for (uint32_t j = deg - 1; j > 0; --j) lam[j] ^= mul(X, lam[j - 1]);
    }
    // row factors log(Dinv_r beta_r^m), log beta_r
    std::vector<uint32_t> lrow(es), lbeta(es);
    for (uint32_t r = 0; r < es; ++r) {
        const uint32_t lb = (255u - (nvecs - 1 - locs[r])) % 255u;
        uint32_t denom = 0;
        for (uint32_t j = 1; j < deg; j += 2)
            if (lam[j]) denom ^= f.exp[(f.log[lam[j]] + (uint64_t)lb * (j - 1)) % 255u];
        const uint32_t ldinv = denom ? (255u - f.log[denom]) % 255u : 0u;  // GINV[0] = 1 (galois.cpp:39)
        lbeta[r] = lb;
        lrow[r] = (ldinv + (m % 255u) * lb) % 255u;
    }
    std::vector<uint8_t> erased(nvecs, 0);
    for (uint32_t i = 0; i < ec; ++i) erased[locs[i]] = 1;
    std::vector<const void*> srcs;
    std::vector<uint32_t> lcols, lgams;
    for (uint32_t v = 0; v < nvecs; ++v) {
        if (erased[v] || !vectors[v]) continue;  // a NULL survivor reads as zeros, as on the GPU
        const uint32_t lgam = (nvecs - 1 - v) % 255u, step = (255u - lgam) % 255u;
        uint32_t acc = 0;
        for (uint32_t i = 0, pi = 0; i <= ec; ++i, pi = (pi + step) % 255u)
            if (lam[i]) acc ^= f.exp[f.log[lam[i]] + pi];
        srcs.push_back(vectors[v]);
        lcols.push_back(((m + 1u) % 255u * lgam + f.log[acc]) % 255u);  // acc != 0: v survived
        lgams.push_back(lgam);
    }
    const uint32_t ncol = (uint32_t)srcs.size();
    std::vector<uint16_t> coef((size_t)es * ncol);
    std::vector<void*> dst(es);
    for (uint32_t r = 0; r < es; ++r) {
        dst[r] = vectors[locs[r]];
        for (uint32_t j = 0; j < ncol; ++j) {
            const uint32_t w1 = f.exp[lgams[j] + lbeta[r]] ^ 1u;  // gamma_v beta_r + 1, nonzero
            coef[(size_t)r * ncol + j] = (uint16_t)f.exp[(lrow[r] + lcols[j] + 255u - f.log[w1]) % 255u];
        }
    }
    return host_rows_apply(false, dst.data(), es, srcs.data(), ncol, coef.data(), c->vec, false);
}

int nfec_decode_vectors_host(nfec_codec* c, void* const* vectors, uint32_t num_data, uint32_t erasure_count,
                             const uint32_t* erasure_locs)
{
    if (!c || !vectors || (erasure_count && !erasure_locs)) return fail(NFEC_EINVAL, "null argument");
    c = primary(c);
    if (c->kind != NFEC_MDP && c->h_lwp.empty())
        return fail(NFEC_ENOTSUP, "host decode: the codec has no closed-form plan constants");
    if (num_data == 0 || num_data > c->k) return fail(NFEC_EINVAL, "numData out of range");
    const uint32_t k = c->k, m = c->m, nd = num_data;
    // the reference's undefined cases (more erasures than parity, unsorted or out-of-range lists)
    // leave the block alone and return 0, as the GPU plans do
    if (erasure_count > m) return 0;
    uint32_t es = 0;
    for (uint32_t i = 0; i < erasure_count; ++i) {
        if (erasure_locs[i] >= nd + m || (i && erasure_locs[i] <= erasure_locs[i - 1])) return 0;
        es += erasure_locs[i] < nd;
    }
    if (es == 0) return (int)erasure_count;  // only parity lost: nothing is filled (:732)
    if (c->kind == NFEC_MDP) {
        const int rc = mdp_decode_host(c, vectors, nd, erasure_count, erasure_locs, es);
        return rc ? rc : (int)erasure_count;
    }
    const bool wide = c->kind == NFEC_RS16;
    const Field& f = wide ? gf16() : gf8();
    const int64_t q = f.q;
    auto md = [&](int64_t v) { v %= q; return v < 0 ? v + q : v; };
    auto L = [&](uint32_t v) { return (int64_t)f.log[v]; };
    // substitute parities: the first es surviving ones in slot order (normEncoderRS8.cpp:689-711)
    std::vector<uint32_t> par;
    {
        uint32_t i = es;  // the parity entries of the sorted list follow the source ones
        for (uint32_t p = 0; p < m && par.size() < es; ++p) {
            if (i < erasure_count && erasure_locs[i] == nd + p) {
                ++i;
                continue;
            }
            par.push_back(p);
        }
        if (par.size() < es) return 0;  // not enough parity
    }
    std::vector<uint32_t> xs(es), yt(es);
    std::vector<uint8_t> erased(nd, 0);
    for (uint32_t s = 0; s < es; ++s) {
        xs[s] = rs_point(f, erasure_locs[s]);
        yt[s] = rs_point(f, k + par[s]);
        erased[erasure_locs[s]] = 1;
    }
    // A^-1[s][t] = exp(lA[s] + lB[t] - log(x_s + y_t)); the map of a received source column j is
    // exp(lA[s] + lC[j] - log(x_s + x_j)) (rs8_plan_rt_kernel's algebra, tests/test_rt_algebra.py)
    std::vector<int64_t> lA(es), lB(es);
    for (uint32_t s = 0; s < es; ++s) {
        int64_t a = c->h_lwp[erasure_locs[s]], b = -(int64_t)c->h_lw[par[s]];
        for (uint32_t t = 0; t < es; ++t) {
            a += L(xs[s] ^ yt[t]);
            b += L(yt[s] ^ xs[t]);
            if (t != s) a -= L(xs[s] ^ xs[t]), b -= L(yt[s] ^ yt[t]);
        }
        lA[s] = md(a);
        lB[s] = md(b);
    }
    // columns: the surviving (non-NULL) source, then the substitute parities (a NULL parity reads
    // as zeros, as in the GPU path)
    std::vector<const void*> srcs;
    std::vector<int64_t> lcol;   // log factor per column
    std::vector<uint32_t> pts;   // its point
    for (uint32_t j = 0; j < nd; ++j) {
        if (erased[j] || !vectors[j]) continue;
        const uint32_t xj = rs_point(f, j);
        int64_t lc = -(int64_t)c->h_lwp[j];
        for (uint32_t t = 0; t < es; ++t) lc += L(xj ^ xs[t]) - L(xj ^ yt[t]);
        srcs.push_back(vectors[j]);
        lcol.push_back(md(lc));
        pts.push_back(xj);
    }
    for (uint32_t t = 0; t < es; ++t) {
        if (!vectors[nd + par[t]]) continue;
        srcs.push_back(vectors[nd + par[t]]);
        lcol.push_back(lB[t]);
        pts.push_back(yt[t]);
    }
    const uint32_t ncol = (uint32_t)srcs.size();
    std::vector<uint16_t> coef((size_t)es * ncol);
    std::vector<void*> dst(es);
    for (uint32_t s = 0; s < es; ++s) {
        dst[s] = vectors[erasure_locs[s]];
        for (uint32_t j = 0; j < ncol; ++j)
            coef[(size_t)s * ncol + j] = (uint16_t)f.exp[md(lA[s] + lcol[j] - L(xs[s] ^ pts[j]))];
    }
    // RS16: an odd last byte is never touched
    const int rc = host_rows_apply(wide, dst.data(), es, srcs.data(), ncol, coef.data(), wide ? c->vec / 2 : c->vec, true);
    return rc ? rc : (int)erasure_count;
}

// Repair products up to which one-block Decode stays on the host, from tools/percall
// (profiles/r04/percall.jsonl): the host path (row dot products, 8 threads past 8 MiB) beat the
// GPU round trip at every measured size -- RS8(128,127) x 8192 B with 100 erasures (105 MB of
// products) 0.36 against 0.79 ms, MDP (209 MB) 0.42 against 0.99 ms, RS16(400,100) with 50
// erasures (14 M symbol products) 0.31 against 0.86 ms -- so the bounds sit a few times past them.
static constexpr uint64_t kHostDecodeRs8Bytes = 256ull << 20;
static constexpr uint64_t kHostDecodeMdpBytes = 512ull << 20;
static constexpr uint64_t kHostDecodeRs16Symbols = 64ull << 20;

int nfec_decode_host_preferred(const nfec_codec* c, uint32_t num_data, uint32_t erasure_count)
{
    if (!c) return 0;
    c = primary(c);
    if (c->host_only) return c->kind == NFEC_MDP || !c->h_lwp.empty() ? 1 : 0;
    const uint64_t e = std::min(erasure_count, c->m);
    // products of the repair: erased rows x columns read x symbols
    if (c->kind == NFEC_MDP) return e * (num_data + c->m) * c->vec <= kHostDecodeMdpBytes ? 1 : 0;
    if (c->h_lwp.empty()) return 0;
    if (c->kind == NFEC_RS8) return e * num_data * c->vec <= kHostDecodeRs8Bytes ? 1 : 0;
    return e * num_data * (c->vec / 2) <= kHostDecodeRs16Symbols ? 1 : 0;
}

int nfec_decode_vectors(nfec_codec* c, void* const* vectors, uint32_t num_data, uint32_t erasure_count,
                        const uint32_t* erasure_locs)
{
    if (!c || !vectors || (erasure_count && !erasure_locs)) return fail(NFEC_EINVAL, "null argument");
    c = primary(c);
    if (c->host_only) return host_only_fail();
    if (num_data == 0 || num_data > c->k) return fail(NFEC_EINVAL, "numData out of range");
    if (erasure_count > c->m) return 0;
    DeviceGuard g(c->device);
    const uint32_t nslots = num_data + c->m;
    // the whole call runs under mu: the staging and the decode workspace are the codec's
    std::lock_guard<std::mutex> lk(c->mu);
    PerCall pc;
    int rc = per_call_stage(c, c->k + c->m, pc);
    if (rc) return rc;
    const hipStream_t st = c->s_stream;
    uint16_t* hl = reinterpret_cast<uint16_t*>(pc.pin + 8);
    std::memset(hl, 0, pc.data0 - 8);
    for (uint32_t i = 0; i < erasure_count; ++i) hl[i] = (uint16_t)erasure_locs[i];
    hl[c->m] = (uint16_t)erasure_count;
    hl[c->m + 1] = (uint16_t)num_data;
    // gather: present vectors as given (erased source arrives zero-filled, normObject.cpp:1579),
    // missing (NULL) parity as zeros
    uint8_t* hp = pc.pin + pc.data0;
    for (uint32_t s = 0; s < nslots; ++s) {
        if (vectors[s]) std::memcpy(hp + (size_t)s * pc.stride, vectors[s], c->vec);
        else std::memset(hp + (size_t)s * pc.stride, 0, c->vec);
    }
    NFEC_HIP(hipMemcpyAsync(pc.dev + 8, pc.pin + 8, pc.data0 - 8 + (size_t)nslots * pc.stride, hipMemcpyHostToDevice, st));
    uint16_t* dl = reinterpret_cast<uint16_t*>(pc.dev + 8);
    int32_t* dstatus = reinterpret_cast<int32_t*>(pc.dev);
    // The reference XORs the repair into the erased buffers (accumulate).  NORM hands them in
    // zero-filled (normObject.cpp:1579), and then overwriting is the same; a full block
    // (numData = k) with zero erased buffers therefore takes the batch fast paths (fused RS8
    // repair, RS16 stages on the tower kernel), anything else the general ones.
    bool zero_erased = true;
    for (uint32_t i = 0; i < erasure_count && zero_erased; ++i) {
        const uint32_t s = erasure_locs[i];
        if (s >= num_data || !vectors[s]) continue;
        const uint8_t* v = static_cast<const uint8_t*>(vectors[s]);
        uint64_t acc = 0, w;
        size_t j = 0;
        for (; j + 8 <= c->vec; j += 8) {
            std::memcpy(&w, v + j, 8);
            acc |= w;
        }
        for (; j < c->vec; ++j) acc |= v[j];
        zero_erased = acc == 0;
    }
    nfec_block_batch b{};
    b.blocks = pc.dev + pc.data0;
    b.block_stride = (uint64_t)(c->k + c->m) * pc.stride;
    b.seg_stride = pc.stride;
    b.nblocks = 1;
    b.num_data = num_data == c->k ? nullptr : dl + c->m + 1;
    b.flags = (c->kind == NFEC_MDP || zero_erased) ? 0 : NFEC_ACCUMULATE;
    if ((rc = decode_device(c, &b, dl, c->m, dl + c->m, dstatus, st, true))) return rc;
    // status and the source slots in one copy (the meta bytes between them ride along)
    NFEC_HIP(hipMemcpyAsync(pc.pin, pc.dev, pc.data0 + (size_t)num_data * pc.stride, hipMemcpyDeviceToHost, st));
    NFEC_HIP(hipStreamSynchronize(st));
    int32_t status;
    std::memcpy(&status, pc.pin, sizeof(status));
    if (status > 0) {
        const size_t out_bytes = c->sym == 2 ? (c->vec & ~1u) : c->vec;  // RS16: odd last byte untouched
        for (uint32_t i = 0; i < erasure_count; ++i) {
            const uint32_t s = erasure_locs[i];
            if (s >= num_data) break;  // parity is never filled (normEncoderRS8.cpp:732)
            if (vectors[s]) std::memcpy(vectors[s], hp + (size_t)s * pc.stride, out_bytes);
        }
    }
    return status;
}

// ---- synthetic workload utilities ----
int nfec_util_fill(const nfec_block_batch* b, uint32_t num_data, uint32_t vector_size, uint64_t seed,
                   uint64_t first_block, void* stream)
{
    if (!b || !b->blocks) return fail(NFEC_EINVAL, "null batch");
    return launch_fill(static_cast<uint8_t*>(b->blocks), b->block_stride, b->seg_stride, b->nblocks, b->num_data,
                       num_data, vector_size, seed, first_block, static_cast<hipStream_t>(stream));
}

int nfec_util_erasures(uint16_t* locs, uint32_t stride, uint16_t* counts, uint32_t nblocks, uint32_t range,
                       uint32_t count, uint64_t seed, uint64_t first_block, void* stream)
{
    if (!locs || !counts || stride == 0) return fail(NFEC_EINVAL, "bad erasure arrays");
    return launch_erasures(locs, stride, counts, nblocks, range, count, seed, first_block,
                           static_cast<hipStream_t>(stream));
}

int nfec_util_zero_slots(const nfec_block_batch* b, const uint16_t* locs, uint32_t stride, const uint16_t* counts,
                         uint32_t vector_size, void* stream)
{
    if (!b || !b->blocks || !locs || !counts) return fail(NFEC_EINVAL, "null argument");
    return launch_zero_slots(static_cast<uint8_t*>(b->blocks), b->block_stride, b->seg_stride, b->nblocks, locs,
                             stride, counts, vector_size, static_cast<hipStream_t>(stream));
}

int nfec_host_threads(uint32_t* pool, uint32_t* usable_cores, uint32_t* visible_cores)
{
    if (pool) *pool = host_pool_workers();
    if (usable_cores) *usable_cores = host_usable_cores();
    if (visible_cores) *visible_cores = host_visible_cores();
    return NFEC_OK;
}

int nfec_util_pool_check(uint32_t pieces, int mode)
{
    if (mode < 0 || mode > 2 || (mode && pieces < 2)) return fail(NFEC_EINVAL, "bad argument");
    std::atomic<uint32_t> ran{0};
    const int rc = host_parallel_for(pieces, [&](unsigned i) {
        if (mode == 1 && i == 1) throw std::bad_alloc();
        if (mode == 2 && i == 1) throw std::runtime_error("pool check");
        ran.fetch_add(1);
    });
    return rc ? rc : (int)ran.load();
}

int nfec_util_stream_copy(void* dst, const void* src, uint64_t bytes, void* stream)
{
    if ((!dst || !src) && bytes) return fail(NFEC_EINVAL, "null argument");
    return launch_stream_copy(dst, src, bytes, static_cast<hipStream_t>(stream));
}

}  // extern "C"
