// codec_state.hpp -- the codec object and what the translation units of the C ABI share:
// nfec_api.cpp (construction, the device and receiver entries, the per-call paths, the host-only
// repair, the utilities), dispatch_encode.cpp and dispatch_decode.cpp (the device-batch
// dispatchers), host_pipeline.cpp (the host-resident batches).  Internal; not installed.
#pragma once

#include <algorithm>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <thread>
#include <vector>

#include "nfec_internal.hpp"

namespace nfec {

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard()
    {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    int reserve(size_t count)
    {
        if (count <= n) return NFEC_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        if (hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(NFEC_ENOMEM, "hipMalloc failed for workspace");
        }
        n = count;
        return NFEC_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

constexpr uint32_t kRowPad = 32;       // coefficient rows padded (kernel row chunk multiple)
// decode blocks per planning pass: bounds the workspace (stage-1 rows z, plan matrices).
// Larger passes measured faster (fewer, fuller launches: 16k -> 64k blocks took
// decode from 2.92 to 2.77 ms per 64k blocks), so a pass is as large as 8 GiB of workspace
// allows (3 % of an MI355X's 288 GB).
// budget_bytes caps it further (decode_pass_size: half of the device memory free plus what the
// codec already holds).  NFEC_SUBBATCH overrides (A/B runs, diagnostic library).
inline uint32_t sub_batch(uint64_t ws_bytes_per_block, uint64_t budget_bytes = 8ull << 30, uint32_t max_blocks = 65536)
{
    static const long env = diag_knob("NFEC_SUBBATCH", 0, 0, 1L << 20);
    if (env > 0) return (uint32_t)std::max(256L, std::min(env, 1L << 20));
    const uint64_t cap = std::min<uint64_t>(8ull << 30, budget_bytes) / std::max<uint64_t>(ws_bytes_per_block, 1);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(max_blocks, cap));
}

inline uint32_t round_up(uint32_t v, uint32_t a) { return (v + a - 1) / a * a; }

}  // namespace nfec

// (every translation unit that includes this header works inside nfec; the codec and request
// types themselves are the C ABI's, so they stay global)
using namespace nfec;

constexpr uint32_t kHostSlots = 3;
struct HostSlot {
    uint8_t* dev = nullptr;
    uint8_t* pin = nullptr;     // pinned staging (pageable callers, segment lists)
    uint8_t* pin_dev = nullptr; // the same staging as the device addresses it (zero-copy kernels)
    uint16_t* dmeta = nullptr;  // num_data, erasure locs, counts
    uint8_t* hmeta = nullptr;   // pinned mirror of dmeta (ChunkMeta)
    int32_t* dstat = nullptr;
    int32_t* hstat = nullptr;   // pinned status readback
    hipStream_t st = nullptr;
    hipEvent_t done = nullptr, ev_up = nullptr, ev_cd = nullptr;
    size_t dev_bytes = 0, pin_bytes = 0, meta_bytes = 0, dstat_bytes = 0, hstat_bytes = 0, hmeta_bytes = 0;
};

// host-batch pipeline resources cached per codec (host_pipeline.cpp: run_chunks claims the slots,
// under nfec_codec::stage_mu)
struct HostStage {
    HostSlot slot[kHostSlots];
    hipStream_t cst = nullptr;  // decode compute stream
    void release()
    {
        for (auto& s : slot) {
            if (s.st) (void)hipStreamSynchronize(s.st);
            if (s.dev) (void)hipFree(s.dev);
            if (s.pin) (void)hipHostFree(s.pin);
            if (s.dmeta) (void)hipFree(s.dmeta);
            if (s.hmeta) (void)hipHostFree(s.hmeta);
            if (s.dstat) (void)hipFree(s.dstat);
            if (s.hstat) (void)hipHostFree(s.hstat);
            if (s.done) (void)hipEventDestroy(s.done);
            if (s.ev_up) (void)hipEventDestroy(s.ev_up);
            if (s.ev_cd) (void)hipEventDestroy(s.ev_cd);
            if (s.st) (void)hipStreamDestroy(s.st);
            s = HostSlot();
        }
        if (cst) {
            (void)hipStreamSynchronize(cst);
            (void)hipStreamDestroy(cst);
            cst = nullptr;
        }
    }
};

// An asynchronous host-batch call (nfec_*_host_vectors_async): the arguments are copied at
// submission, a codec-owned worker thread runs the call, the caller polls or waits.
struct nfec_request {
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;
    int rc = NFEC_OK;
    std::string err;  // the worker thread's error message, handed to the waiting thread
    std::function<int()> run;
};

// One worker thread per codec that has seen an async call: requests on a codec complete in
// submission order (they share the codec's staging pipeline anyway); codecs run concurrently,
// so a receiver with one decoder per remote sender (normNode.h:649) overlaps its senders.
struct AsyncQueue {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<nfec_request*> q;
    std::thread th;
    bool stop = false;
    int device = 0;

    void loop()
    {
        (void)hipSetDevice(device);
        for (;;) {
            nfec_request* r = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || !q.empty(); });
                if (q.empty()) return;  // stop requested and drained
                r = q.front();
                q.pop_front();
            }
            const int rc = r->run();
            std::lock_guard<std::mutex> lk(r->mu);
            if (rc < 0) r->err = last_error_cstr();
            r->rc = rc;
            r->done = true;
            r->cv.notify_all();
        }
    }
    void submit(nfec_request* r)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!th.joinable()) th = std::thread([this] { loop(); });
        q.push_back(r);
        cv.notify_one();
    }
    // finishes every queued request, then stops the thread
    void shutdown()
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
            cv.notify_all();
        }
        if (th.joinable()) th.join();
    }
};

// decode workspace of a codec (guarded by nfec_codec::mu): the plans' outputs, the stage-1 rows z
// and the lists nfec_decode_received builds, sized per pass by decode_reserve
struct DecodeWorkspace {
    DevBuf<int32_t> status, rows, rows1;
    DevBuf<uint32_t> rmax;
    DevBuf<uint16_t> islots, oslots, cols;
    DevBuf<uint8_t> coef1, coef2, z, work, pmap;
    DevBuf<uint32_t> emask, psel, gate;
    DevBuf<uint16_t> tw2;        // RS16 decode stage 2 on the tower kernel: per-block tables
    DevBuf<uint32_t> rowoff;     // ... and output row offsets (TwDecTablesArgs)
    uint32_t gate_gen = 0;       // per-pass generation written into gate (RsPlan2Args)
    DevBuf<uint16_t> rxlocs, rxcounts;  // nfec_decode_received: the lists built from the mask ([b][m], [b])
    // on the codec's device (the destructor's DeviceGuard)
    void release()
    {
        for (auto* b : {&status, &rows, &rows1}) b->release();
        for (auto* b : {&rmax, &emask, &psel, &gate, &rowoff}) b->release();
        for (auto* b : {&islots, &oslots, &cols, &tw2, &rxlocs, &rxcounts}) b->release();
        for (auto* b : {&coef1, &coef2, &z, &work, &pmap}) b->release();
    }
};

struct nfec_codec {
    int kind = 0;
    int device = 0;
    uint32_t opts = 0;  // NFEC_OPT_* (nfec_codec_create_ex)
    uint32_t k = 0, m = 0, vec = 0, sym = 1;
    // a codec over several devices (nfec_codec_create_ex): one full single-device codec per
    // listed device.  Host batches are striped over them in contiguous block ranges; device
    // batches run on the stripe of the batch's device; per-call work on stripe 0.  The outer
    // codec keeps the shape and the generator but no device state.
    std::vector<std::unique_ptr<nfec_codec>> stripes;
    uint32_t cs = 0;  // padded parity-row count
    std::vector<uint32_t> gen;  // m x k parity rows (RS) / LFSR map for a full block (MDP)
    std::vector<uint8_t> mdp_g; // MDP generator polynomial g[0..m] (the host per-segment step)

    // device-resident state
    DevBuf<uint8_t> d_coef;      // encode coefficients, column-major [k][cs] elements
    DevBuf<uint8_t> d_gen;       // m x k row-major elements (decode plan gathers)
    DevBuf<uint32_t> d_vtab;     // 256 x 8 dwords (GF(2^8) kernels)
    DevBuf<uint8_t> d_exp;       // field exp table (2q elements)
    DevBuf<uint16_t> d_log;      // field log table (q+1)
    DevBuf<uint8_t> d_mdp_step;  // MDP single LFSR step matrix, column-major [m+1][cs]
    DevBuf<uint16_t> d_lwp, d_lw;  // RS8 closed-form plan constants: log W'(x_j), log W(y_p)
    std::vector<uint16_t> h_lwp, h_lw;  // the same on the host (nfec_decode_vectors_host)
    // RS8 / MDP products with runtime coefficients (gen_rs8_rt.hip): the generator as snippet
    // offsets [k][m] (RS8), or one [k][m] table per block length nd = 1..k (MDP, shortened)
    DevBuf<uint16_t> d_rt;
    uint64_t rt_block_bytes = 0;   // MDP: bytes per numData table
    DevBuf<uint16_t> d_sel16;      // RS16 bit-sliced encode table offsets [k][m][64] (may be absent)
    DevBuf<uint16_t> d_t3off;      // RS16 shared-table encode LDS offsets [k+1][m_pad][48]
    // RS16 products by the tower-field kernel (gen_gf16_tw.hip) instead of the shared-table one:
    // snippet offsets [k][sweep][m][2] (gf16_tw_table_elems); the Toeplitz split's products likewise
    bool tw = false;
    // NFEC_OPT_HOST_ONLY: no device, no device tables; only the host per-call paths run
    bool host_only = false;
    DevBuf<uint16_t> d_twoff, d_tmvp_tw;
    // RS16 encode by the Toeplitz split (kernels_tmvp.hip): offsets of the three products, each
    // [k/2+1][m_pad(m/2)][48], then the constants' row masks (c_j [k][16], W [m][16], G0 [m][16])
    bool tmvp = false;
    int tmvp_levels = 0;           // Karatsuba levels of the split: 1 (3 products) or 2 (9, tower kernel)
    DevBuf<uint16_t> d_tmvp_off, d_tmvp_mat;
    std::mutex tmvp_mu;            // one Toeplitz encode at a time per codec: they share w_tmvp
    DevBuf<uint8_t> w_tmvp;        // prescaled pair sums + P1 rows of a sub-batch
    hipEvent_t tmvp_done = nullptr;  // the last Toeplitz encode's end, on its stream
    // two-level encode pipeline (rs16_tmvp2_encode): a second stream of the codec's own and the
    // events that fork it from the caller's stream, stagger the sub-batches' prescales and join
    hipStream_t tmvp_s2 = nullptr;
    hipEvent_t tmvp_ev[4] = {};      // fork, join, prescale done (two, alternating)
    // device-batch encodes per path that took them (NFEC_PATH_*, nfec_codec_encode_paths)
    std::atomic<uint64_t> enc_paths[NFEC_PATH_COUNT] = {};
    std::atomic<uint64_t> dec_paths[NFEC_DPATH_COUNT] = {};  // ... and decodes (NFEC_DPATH_*)
    // device batches whose last vec % 8 bytes ran on the tail kernels (encodes, decodes)
    std::atomic<uint64_t> tail_batches[2] = {};

    // decode workspace (guarded by mu)
    std::mutex mu;
    DecodeWorkspace ws;
    // per-call staging (nfec_encode_segment / nfec_decode_vectors, guarded by mu): one device
    // buffer and one pinned mirror of the same layout, and a stream of the codec's own, so a
    // call is one gather, one H2D, the kernels, one D2H and one scatter
    DevBuf<uint8_t> s_block;
    uint8_t* s_pin = nullptr;
    size_t s_pin_bytes = 0;
    hipStream_t s_stream = nullptr;
    // host-batch pipelines (slots, pinned staging, streams): one host-batch call at a time per
    // codec.  Separate from mu, which the decode kernels' workspace takes inside such a call.
    std::mutex stage_mu;
    HostStage stage;
    AsyncQueue async;

    ~nfec_codec()
    {
        async.shutdown();  // outstanding async requests complete before the codec goes away
        // a host-only codec (device -1) holds no device state and never starts the HIP runtime
        // (hipSetDevice(-1) would also leave an error in this thread's last-error slot)
        if (host_only || device < 0) return;
        DeviceGuard g(device);
        stage.release();
        ws.release();
        for (auto* b : {&d_coef, &d_gen, &d_exp, &s_block, &d_mdp_step, &w_tmvp}) b->release();
        d_vtab.release();
        for (auto* b : {&d_log, &d_lwp, &d_lw, &d_rt, &d_sel16, &d_t3off, &d_twoff, &d_tmvp_tw, &d_tmvp_off, &d_tmvp_mat})
            b->release();
        if (s_stream) {
            (void)hipStreamSynchronize(s_stream);
            (void)hipStreamDestroy(s_stream);
        }
        if (s_pin) (void)hipHostFree(s_pin);
        if (tmvp_done) (void)hipEventDestroy(tmvp_done);
        if (tmvp_s2) {
            (void)hipStreamSynchronize(tmvp_s2);
            (void)hipStreamDestroy(tmvp_s2);
        }
        for (hipEvent_t ev : tmvp_ev)
            if (ev) (void)hipEventDestroy(ev);
    }
};

namespace nfec {

// ---- shared between the translation units ----
// the codec that runs per-call work and answers shape queries
inline const nfec_codec* primary(const nfec_codec* c) { return c->stripes.empty() ? c : c->stripes[0].get(); }
inline nfec_codec* primary(nfec_codec* c) { return c->stripes.empty() ? c : c->stripes[0].get(); }
int host_only_fail();  // NFEC_EDEVICE: the codec was created with NFEC_OPT_HOST_ONLY
int check_batch(const nfec_codec* c, const nfec_block_batch* b);
// knobs (diagnostic library; the product takes the defaults): NFEC_FORCE_GENERIC, NFEC_BS_FLAGS,
// NFEC_Q4, NFEC_ASM, NFEC_GF16_T3, NFEC_RS16_TW (nfec_api.cpp)
bool force_generic();
bool has_bitsliced(uint32_t k, uint32_t m);
uint32_t bs_flags();
bool use_q4();
bool use_asm();
bool use_gf16_t3();
bool use_gf16_tw(const nfec_codec* c);
// one RS16 product (encode, decode stage 1) on the codec's product kernel
inline int launch_rs16_product(const nfec_codec* c, const Gf16T3Args& t, hipStream_t s)
{
    return c->tw ? launch_gf16_tw_encode(t, s) : launch_gf16_t3_encode(t, s);
}
// one RS16 product on the tower kernel over a whole vector of any even size (dispatch_encode.cpp)
bool rs16_tw_full_covers(const Gf16T3Args& t);
int launch_rs16_tw_full(const Gf16T3Args& t, hipStream_t s);

// device-batch dispatch: count the batch by the path that took it (dispatch_encode.cpp,
// dispatch_decode.cpp).  caller_locked: the caller already holds c->mu (nfec_decode_vectors
// keeps it for the whole per-call decode, staging included)
int encode_device(nfec_codec* c, const nfec_block_batch* b, hipStream_t s);
int decode_device(nfec_codec* c, const nfec_block_batch* b, const uint16_t* locs, uint32_t lstride,
                  const uint16_t* counts, int32_t* status, hipStream_t s, bool caller_locked = false);

}  // namespace nfec
