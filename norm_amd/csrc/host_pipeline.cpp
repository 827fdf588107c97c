// host_pipeline.cpp -- host-resident batches (nfec_encode_host / nfec_decode_host, the segment-list
// forms nfec_*_host_vectors and their _async twins): pinned staging and a pipeline of device
// slots, each on its own stream, with the upload, the kernels and the download of chunk i
// overlapping chunk i+1's.  run_chunks is the pipeline; run_host_batch (strided blocks) and
// run_host_vectors (NORM's segment-pointer lists) tell it how a chunk's bytes reach a slot and
// how they leave it.  Only the bytes the operation reads go up and only the bytes it writes
// come down:
//   encode  (unshortened, overwrite): up source slots [0,k), down parity slots [k,k+m)
//   encode  (shortened or accumulate): up/down the whole block span
//   decode: zero-copy slot moves (launch_slot_move) of the slots the decode reads and of the
//           repaired ones; without the host mapping, up a window of the span and down source
//           slots [0,k) by DMA (unerased bytes come back unchanged; parity is never written).
// A pinned (page-locked / hipHostRegister'ed) caller buffer is addressed directly; a pageable one
// and the segment lists go through pinned staging, copied by the process's host pool.
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "codec_state.hpp"

namespace {

// pinned host memory as the device addresses it (kernels read and write it over PCIe)
struct HostPtr {
    bool pinned = false;
    uint8_t* dev = nullptr;
};

HostPtr host_ptr(const void* p)
{
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeHost) {
        (void)hipGetLastError();
        return {};
    }
    return {true, static_cast<uint8_t*>(at.devicePointer)};
}

// fn(first, end) over [0, n), cut into pieces of at least 4 MiB: as many as the process's host
// pool has workers, which every concurrent call (and stripe) shares
template <typename F>
int parallel_ranges(uint32_t n, uint64_t bytes, F fn)
{
    const unsigned nt = (unsigned)std::min<uint64_t>(std::min<uint64_t>(host_pool_size(), n),
                                                      std::max<uint64_t>(1, bytes >> 22));
    if (nt <= 1) {
        fn(0u, n);
        return NFEC_OK;
    }
    const uint32_t per = (n + nt - 1) / nt;
    return host_parallel_for(nt, [&](unsigned t) {
        const uint32_t lo = std::min<uint32_t>(n, t * per), hi = std::min<uint32_t>(n, lo + per);
        if (lo < hi) fn(lo, hi);
    });
}

// rows x width bytes, strided on both sides
int copy2d(uint8_t* dst, uint64_t dpitch, const uint8_t* src, uint64_t spitch, uint64_t width, uint32_t rows)
{
    if (rows == 0 || width == 0) return NFEC_OK;
    return parallel_ranges(rows, width * rows, [=](uint32_t r0, uint32_t r1) {
        if (dpitch == width && spitch == width) {
            std::memcpy(dst + r0 * width, src + r0 * width, (size_t)(r1 - r0) * width);
            return;
        }
        for (uint32_t r = r0; r < r1; ++r) std::memcpy(dst + r * dpitch, src + r * spitch, (size_t)width);
    });
}

// the segment-list gather of blocks [b0, b0 + nb): block b's slots [0, numData_b + extra) from
// its pointer list (vecs[b * n + s]; NULL: zero) into dst + (b - b0) * dbs + s * ss.
// extra: m when the parity is read too (decode, accumulate), else 0.
int gather_segments(uint8_t* dst, uint64_t dbs, uint64_t ss, void* const* vecs, uint32_t n, uint32_t b0, uint32_t nb,
                    const uint16_t* num_data, uint32_t k, uint32_t extra, uint32_t vec)
{
    return parallel_ranges(nb, (uint64_t)nb * n * vec, [&](uint32_t i0, uint32_t i1) {
        for (uint32_t i = i0; i < i1; ++i) {
            const uint32_t b = b0 + i;
            const uint32_t up = (num_data ? num_data[b] : k) + extra;
            uint8_t* d = dst + (uint64_t)i * dbs;
            for (uint32_t q = 0; q < up; ++q) {
                const void* p = vecs[(uint64_t)b * n + q];
                if (p) std::memcpy(d + q * ss, p, vec);
                else std::memset(d + q * ss, 0, vec);
            }
        }
    });
}

// ---- cached host staging ----
// The pipeline's device slots, pinned staging, streams and events live in the codec and grow
// on demand: allocating (and freeing, which synchronises the whole device) per call would
// stall every other codec's work on the GPU -- two codecs driven from two host threads (the
// mixed RS8/RS16 stream of BASELINE C5) would serialise.  Host-batch calls on one codec are
// serialised by the codec's stage_mu (the reference's codec instances are single-threaded,
// normApi.cpp:55,126; here concurrent callers of one codec wait rather than race).
int grow_dev(void** p, size_t& cap, size_t need)
{
    if (cap >= need) return NFEC_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    cap = 0;
    if (hipMalloc(p, need) != hipSuccess) return fail(NFEC_ENOMEM, "staging allocation failed");
    cap = need;
    return NFEC_OK;
}

int grow_pin(void** p, size_t& cap, size_t need)
{
    if (cap >= need) return NFEC_OK;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr;
    cap = 0;
    if (hipHostMalloc(p, need, hipHostMallocDefault) != hipSuccess) return fail(NFEC_ENOMEM, "pinned staging allocation failed");
    cap = need;
    return NFEC_OK;
}

int stage_slot(nfec_codec* c, uint32_t i, size_t dev_bytes, size_t pin_bytes, size_t meta_bytes, size_t stat_bytes,
               HostSlot*& out)
{
    HostSlot& s = c->stage.slot[i];
    int rc;
    const uint8_t* pin_before = s.pin;
    if ((rc = grow_dev(reinterpret_cast<void**>(&s.dev), s.dev_bytes, dev_bytes)) ||
        (pin_bytes && (rc = grow_pin(reinterpret_cast<void**>(&s.pin), s.pin_bytes, pin_bytes))) ||
        (rc = grow_dev(reinterpret_cast<void**>(&s.dmeta), s.meta_bytes, meta_bytes)) ||
        (rc = grow_pin(reinterpret_cast<void**>(&s.hmeta), s.hmeta_bytes, meta_bytes)) ||
        (rc = grow_dev(reinterpret_cast<void**>(&s.dstat), s.dstat_bytes, stat_bytes)) ||
        (rc = grow_pin(reinterpret_cast<void**>(&s.hstat), s.hstat_bytes, stat_bytes)))
        return rc;
    if (s.pin != pin_before) s.pin_dev = s.pin ? host_ptr(s.pin).dev : nullptr;
    if (!s.st) {
        const hipError_t se = hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking);
        if (se != hipSuccess ||
            hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s.ev_up, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s.ev_cd, hipEventDisableTiming) != hipSuccess)
            return fail(NFEC_ENOMEM, "staging stream creation failed");
    }
    if (!c->stage.cst) {
        // the decode kernels run at the highest stream priority: the slot moves of the other
        // chunks are PCIe-bound and must not hold the CUs the compute waits for
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) {
            (void)hipGetLastError();
            greatest = 0;
        }
        if (hipStreamCreateWithPriority(&c->stage.cst, hipStreamNonBlocking, greatest) != hipSuccess)
            return fail(NFEC_ENOMEM, "staging stream creation failed");
    }
    out = &s;
    return NFEC_OK;
}

// Blocks per pipeline chunk: about 128 MiB (RS8(64,32) x 1400 B, 65,536 pinned blocks: 1,024-block
// chunks 22.98 GiB/s, 2,048 22.7, 4,096 22.55, 512 21.68 on one box), but never fewer than the blocks it takes to fill
// the GPU when the kernels run one wave per block (RS16, MDP, the generic RS8 kernels: 16 waves
// per CU, 4096 blocks), and at most 4 GiB per slot.
uint32_t host_chunk(const nfec_codec* c, uint64_t dbs, uint32_t nblocks)
{
    if (const char* e = std::getenv("NFEC_HOST_CHUNK_BLOCKS"))  // tests: force multi-chunk pipelines
        if (std::atol(e) > 0) return (uint32_t)std::min<uint64_t>((uint64_t)std::atol(e), nblocks);
    const bool per_block = !(c->kind == NFEC_RS8 && has_bitsliced(c->k, c->m));
    uint64_t ch = std::max<uint64_t>(1, (128ull << 20) / std::max<uint64_t>(dbs, 1));
    if (per_block) ch = std::max<uint64_t>(ch, 4096);
    ch = std::min<uint64_t>(ch, std::max<uint64_t>(1, (4ull << 30) / std::max<uint64_t>(dbs, 1)));
    return (uint32_t)std::min<uint64_t>(ch, nblocks);
}

void stage_drain(nfec_codec* c)
{
    for (auto& s : c->stage.slot)
        if (s.st) (void)hipStreamSynchronize(s.st);
    if (c->stage.cst) (void)hipStreamSynchronize(c->stage.cst);
}

// what a host batch is asked to do, in either form; the arrays are the caller's, on the host
struct HostCall {
    const uint16_t* num_data;  // per block, or null: every block holds k
    const uint16_t* locs;      // decode: erasure lists [nblocks][lstride] and their lengths
    uint32_t lstride;
    const uint16_t* counts;
    int32_t* status;  // decode: per-block result for the caller, or null
    uint32_t flags;   // NFEC_ACCUMULATE
    bool decode;
};

// numData is on the host here: reject what no block of k + m slots can hold before any transfer
// is sized from it
bool num_data_ok(const nfec_codec* c, uint32_t nd) { return nd != 0 && nd <= c->k; }

// A chunk's metadata in its slot's dmeta: numData [chunk], then the erasure lists
// [chunk][lstride], then their counts [chunk].  It goes up through the slot's pinned mirror: an
// async copy straight from the caller's pageable arrays is staged by the runtime and blocks the
// host thread until the link drains, which stalls the pipeline behind the other chunks'
// transfers.  (The slot is reused only after its previous chunk completed.)
struct ChunkMeta {
    uint16_t *nd, *locs, *counts;  // device addresses; nd: null when the batch is unshortened
    static size_t bytes(uint32_t chunk, uint32_t lstride) { return (size_t)chunk * (1 + lstride + 1) * 2 + 16; }
    ChunkMeta(const HostSlot& s, const HostCall& a, uint32_t chunk)
        : nd(a.num_data ? s.dmeta : nullptr), locs(s.dmeta + chunk), counts(locs + (size_t)chunk * a.lstride)
    {
    }
    static hipError_t meta_up(HostSlot& s, uint16_t* dev, const uint16_t* src, size_t count)
    {
        const size_t off = reinterpret_cast<uint8_t*>(dev) - reinterpret_cast<uint8_t*>(s.dmeta);
        std::memcpy(s.hmeta + off, src, count * 2);
        return hipMemcpyAsync(dev, s.hmeta + off, count * 2, hipMemcpyHostToDevice, s.st);
    }
    // blocks [b0, b0 + nb) of the call, on the slot stream; ae: the chunk's upload so far
    hipError_t upload(HostSlot& s, const HostCall& a, uint32_t b0, uint32_t nb, hipError_t ae = hipSuccess) const
    {
        if (ae == hipSuccess && nd) ae = meta_up(s, nd, a.num_data + b0, nb);
        if (ae == hipSuccess && a.decode) ae = meta_up(s, locs, a.locs + (uint64_t)b0 * a.lstride, (size_t)nb * a.lstride);
        if (ae == hipSuccess && a.decode) ae = meta_up(s, counts, a.counts + b0, nb);
        return ae;
    }
};

// Blocks whose numData (known on the host) equals k go to the unshortened fast kernels in
// sub-batches of their own; only the others carry their numData.  NORM batches are mostly full
// blocks with one short block ending each object, and one short block would otherwise send the
// whole batch down the generic (numData-aware) kernels.  Full runs shorter than kMinFullRun stay
// with their neighbours: a launch per handful of blocks costs more than it saves.
template <typename F>
int split_full_runs(const uint16_t* hnd, uint32_t n, uint32_t k, F launch)
{
    constexpr uint32_t kMinFullRun = 32;
    if (!hnd) return launch(0u, n, false);
    uint32_t i = 0;
    while (i < n) {
        uint32_t rs = n, re = n;
        for (uint32_t j = i; j < n;) {
            if (hnd[j] != k) {
                ++j;
                continue;
            }
            uint32_t e = j;
            while (e < n && hnd[e] == k) ++e;
            if (e - j >= kMinFullRun) {
                rs = j;
                re = e;
                break;
            }
            j = e;
        }
        int rc;
        if (rs > i && (rc = launch(i, rs - i, true))) return rc;
        if (rs < n && (rc = launch(rs, re - rs, false))) return rc;
        i = re;
    }
    return NFEC_OK;
}

// The codec's decode workspace (plan, z rows, inverses) is shared by all of its decode calls,
// so every chunk's decode runs on one compute stream: slot stream upload -> event ->
// compute-stream decode -> event -> slot stream download.
int decode_serialized(nfec_codec* c, const nfec_block_batch* db, const uint16_t* dl, uint32_t lstride,
                      const uint16_t* dc, HostSlot& s, uint32_t status_off)
{
    NFEC_HIP(hipEventRecord(s.ev_up, s.st));
    NFEC_HIP(hipStreamWaitEvent(c->stage.cst, s.ev_up, 0));
    const int rc = decode_device(c, db, dl, lstride, dc, s.dstat + status_off, c->stage.cst);
    if (rc) return rc;
    NFEC_HIP(hipEventRecord(s.ev_cd, c->stage.cst));
    NFEC_HIP(hipStreamWaitEvent(s.st, s.ev_cd, 0));
    return NFEC_OK;
}

// The kernels of blocks [b0, b0 + nb) of the call, staged in s.dev at pitches dbs / ss: one
// device batch per run of split_full_runs.  Encode reads only the codec's constants and runs on
// the slot stream; decode on the compute stream, its status at the sub-batch's offset.
int run_kernels(nfec_codec* c, const HostCall& a, HostSlot& s, const ChunkMeta& dm, uint32_t b0, uint32_t nb,
                uint64_t dbs, uint64_t ss)
{
    return split_full_runs(a.num_data ? a.num_data + b0 : nullptr, nb, c->k, [&](uint32_t o, uint32_t n, bool nd) {
        nfec_block_batch sb{};
        sb.blocks = s.dev + o * dbs;
        sb.block_stride = dbs;
        sb.seg_stride = (uint32_t)ss;
        sb.nblocks = n;
        sb.num_data = nd ? dm.nd + o : nullptr;
        sb.flags = a.flags;
        return a.decode ? decode_serialized(c, &sb, dm.locs + (uint64_t)o * a.lstride, a.lstride, dm.counts + o, s, o)
                        : encode_device(c, &sb, s.st);
    });
}

// Decode moves its bytes by zero-copy kernels where the device can address the host side of the
// move: up only the slots the decode reads (surviving source + the first e surviving parities;
// an erased source slot only when accumulating), down only the repaired source slots of blocks
// with status > 0.  Per RS8(64,32) block with 16 source erasures that is 64 segments up and 16
// down, against 80 and 64 for the window DMA, which stays for encode and for setups where the
// host memory is not mapped.  host_dev is the host side as the device addresses it:
//
//   caller's buffer      host_dev                          k + m <= 65,536   k + m > 65,536
//   pinned               its mapped address, if it has one  zero-copy         window DMA
//   pinned, not mapped   null                               window DMA        window DMA
//   pageable, or a list  the slot's pin_dev, if mapped      zero-copy         window DMA
//   ... staging not mapped: null                            window DMA        window DMA
//
// and encode never.  (The slot kernels index a block's slots in 16 bits.)  NFEC_HOST_ZC=0
// (diagnostic library, read per call) turns it off, so that tests reach the window DMA.
bool zero_copy(const nfec_codec* c, const HostCall& a, const uint8_t* host_dev)
{
    return a.decode && host_dev && (uint64_t)c->k + c->m <= 65536 && diag_knob("NFEC_HOST_ZC", 1) != 0;
}

// the gather of a chunk's read slots from host memory (src: as the device addresses it, at
// pitches src_block_stride / ss) into the slot's device buffer ...
SlotMoveArgs slots_in(const nfec_codec* c, const HostCall& a, const HostSlot& s, const ChunkMeta& dm, uint32_t nb,
                      const uint8_t* src, uint64_t src_block_stride, uint64_t dbs, uint64_t ss)
{
    SlotMoveArgs mv;
    mv.src = src;
    mv.src_block_stride = src_block_stride;
    mv.src_seg_stride = (uint32_t)ss;
    mv.dst = s.dev;
    mv.dst_block_stride = dbs;
    mv.dst_seg_stride = (uint32_t)ss;
    mv.nblocks = nb;
    mv.k = c->k;
    mv.m = c->m;
    mv.bytes = c->vec;
    mv.num_data = dm.nd;
    mv.locs = dm.locs;
    mv.lstride = a.lstride;
    mv.counts = dm.counts;
    mv.mode = c->kind == NFEC_MDP ? SLOTS_ALL_IN : SLOTS_RS_IN;
    mv.accumulate = (a.flags & NFEC_ACCUMULATE) ? 1u : 0u;
    return mv;
}

// ... and the scatter of the repaired source slots back the same way (RS16 never writes an odd
// last byte, normEncoderRS16.cpp:733)
SlotMoveArgs slots_out(const nfec_codec* c, const SlotMoveArgs& in, const HostSlot& s)
{
    SlotMoveArgs mv = in;
    mv.src = in.dst;
    mv.src_block_stride = in.dst_block_stride;
    mv.dst = const_cast<uint8_t*>(in.src);  // the caller's blocks or the slot's staging: writable
    mv.dst_block_stride = in.src_block_stride;
    mv.bytes = c->sym == 2 ? (c->vec & ~1u) : c->vec;
    mv.status = s.dstat;
    mv.mode = SLOTS_OUT;
    return mv;
}

// One chunk on a slot: blocks [b0, b0 + nb) of the call; dl: a decode's download length, for
// the collect
struct Job {
    uint32_t b0 = 0, nb = 0;
    uint64_t dl = 0;
    bool busy = false;
};

// The pipeline: nblocks blocks of dbs staged bytes each, in chunks over up to kHostSlots slots.
// issue(slot, job, chunk) enqueues the job's uploads, kernels and downloads on the slot's stream
// and records slot.done; collect(slot, job) runs after that event and hands the chunk's bytes to
// the caller.  A slot takes its next chunk only after its previous one was collected.  One
// host-batch call at a time per codec (stage_mu, held throughout; the caller has set the
// device).  Every error after the first enqueue drains the streams before it returns.
// stage_pin: the slots need pinned staging; what: names the call in a late error.
template <typename Issue, typename Collect>
int run_chunks(nfec_codec* c, const HostCall& a, uint32_t nblocks, uint64_t dbs, bool stage_pin, const char* what,
               Issue issue, Collect collect)
{
    std::lock_guard<std::mutex> stage_lock(c->stage_mu);
    const uint32_t chunk = host_chunk(c, dbs, nblocks);
    const uint32_t used = std::min<uint32_t>(kHostSlots, (nblocks + chunk - 1) / chunk);
    HostSlot* sl[kHostSlots] = {};
    int rc;
    for (uint32_t i = 0; i < used; ++i)
        if ((rc = stage_slot(c, i, (size_t)chunk * dbs, stage_pin ? (size_t)chunk * dbs : 0,
                             ChunkMeta::bytes(chunk, a.lstride), (size_t)chunk * 4 + 16, sl[i])))
            return rc;
    Job jobs[kHostSlots];
    auto finish = [&](uint32_t i) -> int {
        Job& j = jobs[i];
        if (!j.busy) return NFEC_OK;
        j.busy = false;
        NFEC_HIP(hipEventSynchronize(sl[i]->done));
        if (const int rc = collect(*sl[i], j)) return rc;
        if (a.status) std::memcpy(a.status + j.b0, sl[i]->hstat, (size_t)j.nb * 4);
        return NFEC_OK;
    };
    auto bail = [&](int code) {
        stage_drain(c);
        return code;
    };
    uint32_t idx = 0;
    for (uint32_t b0 = 0; b0 < nblocks; b0 += chunk, ++idx) {
        const uint32_t i = idx % used;
        if ((rc = finish(i))) return bail(rc);
        Job& j = jobs[i];
        j.b0 = b0;
        j.nb = std::min(chunk, nblocks - b0);
        if ((rc = issue(*sl[i], j, chunk))) return bail(rc);
        j.busy = true;
    }
    for (uint32_t q = 0; q < used; ++q)
        if ((rc = finish((idx + q) % used))) return bail(rc);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return bail(hip_fail(e, what));
    return NFEC_OK;
}

// A host batch on a codec over several devices: contiguous block ranges [i*B/N, (i+1)*B/N), one
// per stripe, each through that stripe's own pipeline on a host thread of its own (SURVEY 8e:
// no exchange between the ranges).  fn(stripe, first block, blocks) runs one range.  The
// first failing range's status and message are returned on the calling thread.
template <typename F>
int run_striped(nfec_codec* c, uint32_t nblocks, F fn)
{
    const uint32_t ns = (uint32_t)std::min<size_t>(c->stripes.size(), std::max(nblocks, 1u));
    std::vector<int> rcs(ns, NFEC_OK);
    std::vector<std::string> errs(ns);
    auto one = [&](uint32_t i) {
        const uint32_t lo = (uint32_t)((uint64_t)nblocks * i / ns), hi = (uint32_t)((uint64_t)nblocks * (i + 1) / ns);
        rcs[i] = hi > lo ? fn(c->stripes[i].get(), lo, hi - lo) : NFEC_OK;
        if (rcs[i] < 0) errs[i] = last_error_cstr();
    };
    // one driver thread per stripe (they mostly wait on their GPU; the copies go to the host pool)
    std::vector<std::thread> th;
    std::vector<uint32_t> inline_ranges;
    for (uint32_t i = 1; i < ns; ++i) {
        try {
            th.emplace_back(one, i);
        } catch (...) {
            inline_ranges.push_back(i);  // no thread to be had: that range on the calling thread
        }
    }
    one(0);
    for (uint32_t i : inline_ranges) one(i);
    for (auto& t : th) t.join();
    for (uint32_t i = 0; i < ns; ++i)
        if (rcs[i] < 0) return fail(rcs[i], errs[i]);
    return NFEC_OK;
}

// the call for blocks [b0, ...) of a striped batch
HostCall sub_call(const HostCall& a, uint32_t b0)
{
    HostCall s = a;
    if (a.num_data) s.num_data += b0;
    if (a.locs) s.locs += (uint64_t)b0 * a.lstride;
    if (a.counts) s.counts += b0;
    if (a.status) s.status += b0;
    return s;
}

// ---- strided blocks ----
int run_host_batch(nfec_codec* c, const nfec_block_batch* hb, HostCall a)
{
    int rc = check_batch(c, hb);
    if (rc || hb->nblocks == 0) return rc;
    a.num_data = hb->num_data;
    a.flags = hb->flags;
    if (!c->stripes.empty())
        return run_striped(c, hb->nblocks, [&](nfec_codec* sc, uint32_t b0, uint32_t nb) {
            nfec_block_batch sub = *hb;
            sub.blocks = static_cast<uint8_t*>(hb->blocks) + (uint64_t)b0 * hb->block_stride;
            sub.nblocks = nb;
            sub.num_data = hb->num_data ? hb->num_data + b0 : nullptr;
            return run_host_batch(sc, &sub, sub_call(a, b0));
        });
    if (hb->num_data)
        for (uint32_t b = 0; b < hb->nblocks; ++b)
            if (!num_data_ok(c, hb->num_data[b])) return fail(NFEC_EINVAL, "num_data out of range");
    DeviceGuard g(c->device);
    const bool decode = a.decode;
    const uint64_t hbs = hb->block_stride;
    const uint64_t ss = hb->seg_stride;
    const uint64_t dbs = (uint64_t)(c->k + c->m) * ss;       // compact device pitch
    const uint64_t span = (uint64_t)(c->k + c->m - 1) * ss + c->vec;  // bytes a block op can touch
    const bool partial_enc = !decode && !(hb->flags & NFEC_ACCUMULATE) && !hb->num_data;
    const uint64_t up_len = partial_enc ? (uint64_t)(c->k - 1) * ss + c->vec : span;
    const uint64_t dn_off = partial_enc ? (uint64_t)c->k * ss : 0;
    const uint64_t dn_len = partial_enc ? (uint64_t)(c->m - 1) * ss + c->vec
                                        : (decode ? (uint64_t)(c->k - 1) * ss + c->vec : span);
    // download pieces: parity slots one by one when slots carry padding (so the caller's
    // bytes between vec and seg_stride are never overwritten)
    std::vector<std::pair<uint64_t, uint64_t>> dn;
    if (partial_enc && ss != c->vec)
        for (uint32_t p = 0; p < c->m; ++p) dn.emplace_back((uint64_t)(c->k + p) * ss, (uint64_t)c->vec);
    else
        dn.emplace_back(dn_off, dn_len);
    uint8_t* const hbase = static_cast<uint8_t*>(hb->blocks);
    const HostPtr hp = host_ptr(hbase);
    const bool pinned = hp.pinned;
    // The window of a decode without the zero-copy moves.  RS decode reads the source slots and
    // only the first e surviving parities of a block (P, normEncoderRS8.cpp:680-700), so a
    // chunk's upload stops after the last parity slot any of
    // its blocks uses: [0, k + 16) instead of the whole span for RS8(64,32) with 16 source
    // erasures.  MDP decode reads every surviving vector (normEncoderMDP.cpp:346-361).
    // The download then covers [0, max numData) of the chunk, which the upload always includes
    // (slots past the upload hold another chunk's bytes and must not travel back).
    auto decode_up_len = [&](uint32_t b0, uint32_t nb, uint64_t& down) -> uint64_t {
        down = dn_len;
        if (c->kind == NFEC_MDP) return span;
        uint32_t top = 0, ndmax = 0;  // slots [0, top) are read by some block of the chunk
        std::vector<uint8_t> erased(c->k + c->m);
        for (uint32_t b = b0; b < b0 + nb; ++b) {
            const uint32_t nd = hb->num_data ? hb->num_data[b] : c->k;
            const uint32_t ec = std::min<uint32_t>(a.counts[b], a.lstride);
            const uint16_t* l = a.locs + (uint64_t)b * a.lstride;
            const uint32_t nvec = nd + c->m;
            if (!num_data_ok(c, nd)) return span;
            ndmax = std::max(ndmax, nd);
            std::fill(erased.begin(), erased.begin() + nvec, 0);
            uint32_t es = 0;
            for (uint32_t i = 0; i < ec; ++i) {
                if (l[i] >= nvec) return span;  // invalid list: the plan rejects it, stay safe
                erased[l[i]] = 1;
                es += l[i] < nd;
            }
            uint32_t used = 0, end = nd;
            for (uint32_t v = nd; v < nvec && used < es; ++v)
                if (!erased[v]) {
                    ++used;
                    end = v + 1;
                }
            if (used < es) return span;  // undecodable: nothing is read, but keep it simple
            top = std::max(top, end);
        }
        down = (uint64_t)(ndmax - 1) * ss + c->vec;
        return (uint64_t)(top - 1) * ss + c->vec;  // top >= ndmax >= 1
    };
    auto issue = [&](HostSlot& s, Job& j, uint32_t chunk) -> int {
        int rc;
        uint8_t* hsrc = hbase + (uint64_t)j.b0 * hbs;
        j.dl = dn_len;
        const uint64_t ul = decode ? decode_up_len(j.b0, j.nb, j.dl) : up_len;
        const ChunkMeta dm(s, a, chunk);
        hipError_t ae;
        // (a pageable caller's chunk goes through the slot's pinned staging, which the zero-copy
        // kernels need device-mapped; where it is not, the window DMA below takes the chunk)
        if (zero_copy(c, a, pinned ? hp.dev : s.pin_dev)) {
            if ((ae = dm.upload(s, a, j.b0, j.nb)) != hipSuccess) return hip_fail(ae, "host decode metadata upload");
            if (!pinned && (rc = copy2d(s.pin, dbs, hsrc, hbs, ul, j.nb))) return rc;
            const SlotMoveArgs in = pinned ? slots_in(c, a, s, dm, j.nb, hp.dev + (uint64_t)j.b0 * hbs, hbs, dbs, ss)
                                           : slots_in(c, a, s, dm, j.nb, s.pin_dev, dbs, dbs, ss);
            if ((rc = launch_slot_move(in, s.st))) return rc;
            // timing probes (diagnostic library): 1 no decode, 2 no scatter, 3 neither.  Measured (16k
            // blocks RS8(64,32), tools/host_rate.py): 33.1 / 29.3 / 29.9 / 29.1 ms; a window DMA for the
            // download instead of the scatter: 51 ms (DMA writes and zero-copy reads share the link badly)
            static const long probe = diag_knob("NFEC_ZC_PROBE", 0, 0, 3);
            if (!(probe & 1) && (rc = run_kernels(c, a, s, dm, j.b0, j.nb, dbs, ss))) return rc;
            if (!(probe & 2) && (rc = launch_slot_move(slots_out(c, in, s), s.st))) return rc;
            ae = hipMemcpyAsync(s.hstat, s.dstat, (size_t)j.nb * 4, hipMemcpyDeviceToHost, s.st);
            if (ae == hipSuccess) ae = hipEventRecord(s.done, s.st);
            return ae == hipSuccess ? NFEC_OK : hip_fail(ae, "host decode status");
        }
        // window up, kernels, window down
        if (pinned) {
            ae = hipMemcpy2DAsync(s.dev, dbs, hsrc, hbs, ul, j.nb, hipMemcpyHostToDevice, s.st);
        } else {
            if ((rc = copy2d(s.pin, dbs, hsrc, hbs, ul, j.nb))) return rc;
            ae = hipMemcpyAsync(s.dev, s.pin, (size_t)(j.nb - 1) * dbs + ul, hipMemcpyHostToDevice, s.st);
        }
        if ((ae = dm.upload(s, a, j.b0, j.nb, ae)) != hipSuccess) return hip_fail(ae, "host batch upload");
        if ((rc = run_kernels(c, a, s, dm, j.b0, j.nb, dbs, ss))) return rc;
        if (pinned)
            for (size_t q = 0; q < dn.size() && ae == hipSuccess; ++q)
                ae = hipMemcpy2DAsync(hsrc + dn[q].first, hbs, s.dev + dn[q].first, dbs, decode ? j.dl : dn[q].second,
                                      j.nb, hipMemcpyDeviceToHost, s.st);
        else
            ae = hipMemcpyAsync(s.pin + dn_off, s.dev + dn_off, (size_t)(j.nb - 1) * dbs + (decode ? j.dl : dn_len),
                                hipMemcpyDeviceToHost, s.st);
        if (ae == hipSuccess && a.status)
            ae = hipMemcpyAsync(s.hstat, s.dstat, (size_t)j.nb * 4, hipMemcpyDeviceToHost, s.st);
        if (ae == hipSuccess) ae = hipEventRecord(s.done, s.st);
        return ae == hipSuccess ? NFEC_OK : hip_fail(ae, "host batch copy");
    };
    auto collect = [&](HostSlot& s, const Job& j) -> int {
        if (!pinned)
            for (const auto& pc : dn)
                if (const int rc = copy2d(hbase + (uint64_t)j.b0 * hbs + pc.first, hbs, s.pin + pc.first, dbs,
                                          decode ? j.dl : pc.second, j.nb))
                    return rc;
        return NFEC_OK;
    };
    return run_chunks(c, a, hb->nblocks, dbs, !pinned, "host batch", issue, collect);
}

// ---- host segment lists (NORM's scattered segment pool) ----
// NormObject::CalculateBlockParity (src/common/normObject.cpp:2203-2229) and the receiver's
// NormSenderNode::Decode path (normObject.cpp:1548-1644) hold a block as a list of segment
// pointers from the segment pool (normSegment.cpp:14-86), not as one strided buffer.  These
// batches gather the listed segments into pinned staging (host threads), run the chunks through
// the pipeline, and scatter back only the bytes the reference writes: parity slots for encode,
// the erased source slots for decode (RS16: the even part of vector_size; an odd last byte is
// never written, normEncoderRS16.cpp:479).
int run_host_vectors(nfec_codec* c, void* const* vecs, uint32_t nblocks, const HostCall& a)
{
    const bool decode = a.decode;
    if (!c || (nblocks && !vecs)) return fail(NFEC_EINVAL, "null codec or vector list");
    if (primary(c)->host_only) return host_only_fail();
    if (decode && (!a.locs || !a.counts || a.lstride == 0)) return fail(NFEC_EINVAL, "bad erasure arrays");
    if (nblocks == 0) return NFEC_OK;
    if (!c->stripes.empty())
        return run_striped(c, nblocks, [&](nfec_codec* sc, uint32_t b0, uint32_t nb) {
            return run_host_vectors(sc, vecs + (uint64_t)b0 * (c->k + c->m), nb, sub_call(a, b0));
        });
    const uint32_t n = c->k + c->m;
    const uint64_t ss = round_up(c->vec, 8u);
    const uint64_t dbs = (uint64_t)n * ss;
    const bool acc = (a.flags & NFEC_ACCUMULATE) != 0;
    const size_t out_bytes = c->sym == 2 ? (c->vec & ~1u) : c->vec;
    // validate the lists (the reference dereferences every source vector and, for encode,
    // every parity vector; decode never touches missing parity, normEncoderRS8.cpp:689-711)
    for (uint32_t b = 0; b < nblocks; ++b) {
        const uint32_t nd = a.num_data ? a.num_data[b] : c->k;
        if (!num_data_ok(c, nd)) return fail(NFEC_EINVAL, "num_data out of range");
        const uint32_t need = decode ? nd : nd + c->m;
        for (uint32_t s = 0; s < need; ++s)
            if (!vecs[(uint64_t)b * n + s]) return fail(NFEC_EINVAL, "null source/parity vector");
    }
    DeviceGuard g(c->device);
    auto issue = [&](HostSlot& s, Job& j, uint32_t chunk) -> int {
        int rc;
        // encode without accumulate reads the source only; everything else reads the whole
        // listed block (absent parity is zero, as MDP's decoder treats it)
        if ((rc = gather_segments(s.pin, dbs, ss, vecs, n, j.b0, j.nb, a.num_data, c->k, (!decode && !acc) ? 0u : c->m,
                                  c->vec)))
            return rc;
        // decode: the staged slots the decode reads go up by the zero-copy gather kernel (the
        // erased source and unused parity stay on the host), the repaired ones come down by
        // the scatter kernel; otherwise the staged chunk travels by DMA
        const bool zc = zero_copy(c, a, s.pin_dev);
        const ChunkMeta dm(s, a, chunk);
        hipError_t ae = dm.upload(s, a, j.b0, j.nb, zc ? hipSuccess : hipMemcpyAsync(s.dev, s.pin, (size_t)j.nb * dbs,
                                                                                    hipMemcpyHostToDevice, s.st));
        if (ae != hipSuccess) return hip_fail(ae, "vector batch upload");
        const SlotMoveArgs in = slots_in(c, a, s, dm, j.nb, s.pin_dev, dbs, dbs, ss);
        if (zc && (rc = launch_slot_move(in, s.st))) return rc;
        if ((rc = run_kernels(c, a, s, dm, j.b0, j.nb, dbs, ss))) return rc;
        if (zc && (rc = launch_slot_move(slots_out(c, in, s), s.st))) return rc;
        if (decode && (ae = hipMemcpyAsync(s.hstat, s.dstat, (size_t)j.nb * 4, hipMemcpyDeviceToHost, s.st)) != hipSuccess)
            return hip_fail(ae, "vector batch status");
        // unshortened encode: only the parity region of each block comes back
        if (zc)
            ae = hipSuccess;
        else if (!decode && !a.num_data)
            ae = hipMemcpy2DAsync(s.pin + (uint64_t)c->k * ss, dbs, s.dev + (uint64_t)c->k * ss, dbs, (uint64_t)c->m * ss,
                                  j.nb, hipMemcpyDeviceToHost, s.st);
        else
            ae = hipMemcpyAsync(s.pin, s.dev, (size_t)j.nb * dbs, hipMemcpyDeviceToHost, s.st);
        if (ae == hipSuccess) ae = hipEventRecord(s.done, s.st);
        return ae == hipSuccess ? NFEC_OK : hip_fail(ae, "vector batch download");
    };
    auto collect = [&](HostSlot& s, const Job& j) {
        return parallel_ranges(j.nb, (uint64_t)j.nb * (uint64_t)c->m * c->vec, [&](uint32_t i0, uint32_t i1) {
            for (uint32_t i = i0; i < i1; ++i) {
                const uint32_t b = j.b0 + i;
                const uint32_t nd = a.num_data ? a.num_data[b] : c->k;
                const uint8_t* src = s.pin + (uint64_t)i * dbs;
                if (!decode) {
                    for (uint32_t p = 0; p < c->m; ++p)
                        std::memcpy(vecs[(uint64_t)b * n + nd + p], src + (nd + p) * ss, out_bytes);
                } else if (s.hstat[i] > 0) {
                    const uint16_t* l = a.locs + (uint64_t)b * a.lstride;
                    for (uint32_t e = 0; e < a.counts[b] && e < a.lstride; ++e) {
                        if (l[e] >= nd) break;  // only source erasures are filled (normEncoderRS8.cpp:732)
                        std::memcpy(vecs[(uint64_t)b * n + l[e]], src + l[e] * ss, out_bytes);
                    }
                }
            }
        });
    };
    return run_chunks(c, a, nblocks, dbs, true, "vector batch", issue, collect);
}

// ---- asynchronous segment-list batches (receiver cross-block batching) ----
// The receiver's decode site (NormObject::HandleObjectMessage -> NormSenderNode::Decode,
// normObject.cpp:1548-1644, normNode.h:484-487) repairs one block per call on the protocol
// thread.  These calls queue many blocks (from one remote sender's decoder) and return at
// once; the protocol thread keeps receiving and collects completions with nfec_request_test /
// nfec_request_wait.  The pointer table, numData, erasure lists and counts are copied at
// submission; the segment buffers and status array must stay valid until completion.
int submit_vectors(nfec_codec* c, void* const* vecs, uint32_t nblocks, HostCall a, nfec_request** out)
{
    if (!out) return fail(NFEC_EINVAL, "null request pointer");
    *out = nullptr;
    if (!c || (nblocks && !vecs)) return fail(NFEC_EINVAL, "null codec or vector list");
    if (primary(c)->host_only) return host_only_fail();
    if (a.decode && (!a.locs || !a.counts || a.lstride == 0)) return fail(NFEC_EINVAL, "bad erasure arrays");
    const uint64_t n = (uint64_t)c->k + c->m;
    auto tab = std::make_shared<std::vector<void*>>(vecs, vecs + n * nblocks);
    auto nd = std::make_shared<std::vector<uint16_t>>();
    if (a.num_data) nd->assign(a.num_data, a.num_data + nblocks);
    auto el = std::make_shared<std::vector<uint16_t>>();
    auto ec = std::make_shared<std::vector<uint16_t>>();
    if (a.decode) {
        el->assign(a.locs, a.locs + (uint64_t)a.lstride * nblocks);
        ec->assign(a.counts, a.counts + nblocks);
    }
    std::unique_ptr<nfec_request> r(new nfec_request);
    r->run = [=]() {
        HostCall own = a;
        own.num_data = a.num_data ? nd->data() : nullptr;
        own.locs = a.decode ? el->data() : nullptr;
        own.counts = a.decode ? ec->data() : nullptr;
        return run_host_vectors(c, tab->data(), nblocks, own);
    };
    c->async.submit(r.get());
    *out = r.release();
    return NFEC_OK;
}

}  // namespace

extern "C" {

int nfec_encode_host_vectors(nfec_codec* codec, void* const* vectors, uint32_t nblocks, const uint16_t* num_data,
                             uint32_t flags)
{
    return run_host_vectors(codec, vectors, nblocks, {num_data, nullptr, 0, nullptr, nullptr, flags, false});
}

int nfec_decode_host_vectors(nfec_codec* codec, void* const* vectors, uint32_t nblocks, const uint16_t* num_data,
                             const uint16_t* erasure_locs, uint32_t erasure_stride, const uint16_t* erasure_counts,
                             int32_t* status, uint32_t flags)
{
    return run_host_vectors(codec, vectors, nblocks,
                            {num_data, erasure_locs, erasure_stride, erasure_counts, status, flags, true});
}

int nfec_encode_host(nfec_codec* codec, const nfec_block_batch* host_batch)
{
    return run_host_batch(codec, host_batch, {nullptr, nullptr, 0, nullptr, nullptr, 0, false});
}

int nfec_decode_host(nfec_codec* codec, const nfec_block_batch* host_batch, const uint16_t* erasure_locs,
                     uint32_t erasure_stride, const uint16_t* erasure_counts, int32_t* status)
{
    if (!erasure_locs || !erasure_counts || erasure_stride == 0) return fail(NFEC_EINVAL, "bad erasure arrays");
    return run_host_batch(codec, host_batch, {nullptr, erasure_locs, erasure_stride, erasure_counts, status, 0, true});
}

int nfec_encode_host_vectors_async(nfec_codec* codec, void* const* vectors, uint32_t nblocks, const uint16_t* num_data,
                                   uint32_t flags, nfec_request** request)
{
    return submit_vectors(codec, vectors, nblocks, {num_data, nullptr, 0, nullptr, nullptr, flags, false}, request);
}

int nfec_decode_host_vectors_async(nfec_codec* codec, void* const* vectors, uint32_t nblocks,
                                   const uint16_t* num_data, const uint16_t* erasure_locs, uint32_t erasure_stride,
                                   const uint16_t* erasure_counts, int32_t* status, uint32_t flags,
                                   nfec_request** request)
{
    return submit_vectors(codec, vectors, nblocks,
                          {num_data, erasure_locs, erasure_stride, erasure_counts, status, flags, true}, request);
}

int nfec_request_test(nfec_request* r)
{
    if (!r) return fail(NFEC_EINVAL, "null request");
    std::lock_guard<std::mutex> lk(r->mu);
    return r->done ? 1 : 0;
}

int nfec_request_wait(nfec_request* r)
{
    if (!r) return fail(NFEC_EINVAL, "null request");
    int rc;
    std::string err;
    {
        std::unique_lock<std::mutex> lk(r->mu);
        r->cv.wait(lk, [&] { return r->done; });
        rc = r->rc;
        err.swap(r->err);
    }
    delete r;
    return rc < 0 ? fail(rc, err) : rc;
}

// host-side rate of the segment-list gather alone, as nstripes stripes would run it (no device)
int nfec_util_gather_probe(void* const* vectors, uint32_t nblocks, uint32_t slots, uint32_t vector_size,
                           uint32_t nstripes, uint32_t reps, double* seconds, uint32_t* max_active)
{
    if (!vectors || !seconds || nblocks == 0 || slots == 0 || vector_size == 0 || nstripes == 0 || nstripes > 64 ||
        reps == 0)
        return fail(NFEC_EINVAL, "bad argument");
    const uint64_t ss = round_up(vector_size, 8u), dbs = (uint64_t)slots * ss;
    const uint32_t chunk = (uint32_t)std::max<uint64_t>(1, (128ull << 20) / dbs);  // the pipelines' 128 MiB chunks
    std::vector<std::unique_ptr<uint8_t, void (*)(void*)>> stage;
    for (uint32_t i = 0; i < nstripes; ++i) {
        const uint64_t nb = (uint64_t)nblocks * (i + 1) / nstripes - (uint64_t)nblocks * i / nstripes;
        void* p = nullptr;
        const size_t bytes = (size_t)std::max<uint64_t>(1, std::min<uint64_t>(nb, chunk)) * dbs;
        if (posix_memalign(&p, 4096, bytes)) return fail(NFEC_ENOMEM, "probe staging");
        std::memset(p, 0, bytes);  // touched before timing
        stage.emplace_back(static_cast<uint8_t*>(p), std::free);
    }
    auto stripe = [&](uint32_t i) {
        const uint32_t lo = (uint32_t)((uint64_t)nblocks * i / nstripes), hi = (uint32_t)((uint64_t)nblocks * (i + 1) / nstripes);
        for (uint32_t b0 = lo; b0 < hi; b0 += chunk)
            (void)gather_segments(stage[i].get(), dbs, ss, vectors, slots, b0, std::min(chunk, hi - b0), nullptr, slots,
                                  0, vector_size);
    };
    auto pass = [&] {
        std::vector<std::thread> th;
        for (uint32_t i = 1; i < nstripes; ++i) th.emplace_back(stripe, i);
        stripe(0);
        for (auto& t : th) t.join();
    };
    pass();  // untimed: first touches of the pool, the table and the staging
    if (max_active) host_pool_max_active(true);
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t r = 0; r < reps; ++r) pass();
    *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / reps;
    if (max_active) *max_active = host_pool_max_active(false);
    return NFEC_OK;
}

}  // extern "C"
