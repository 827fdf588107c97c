// segment_copy_asan.cpp -- the two misaligned-copy rules of the tx, rx and object kernels
// (norm_amd/csrc/segment_copy.hpp) on the host, under AddressSanitizer and UBSan, with every byte
// outside what a rule may touch poisoned: a load outside the aligned chunks that hold the source, a
// load past a slot's last 8-byte chunk or a store outside the destination bytes stops the run.  The
// kernels compare output bytes only; an over-read inside an allocation changes none, so this is the
// check of what the header's comments claim.  Host code only, no GPU; `make -C tests/native
// -f segment_copy_asan.mk`.
//
// The lanes of a wave run one after the other.  Two walks, as the kernels make them: one source per
// wave, lane L taking pieces L, L + 64, ... (place_segment, emit_message), and 256 lanes striding
// over the (segment, piece) pairs of a run of segments as one flat index (obj_read_kernel,
// obj_write_kernel), where a gather piece takes its second chunk from the next lane.
//
// ASan poisons whole 8-byte granules or their tails.  The bytes between a destination's 8-byte
// granule and an unaligned dst[0] therefore stay addressable; a store there is caught by comparing
// every byte around the destination with what it held before.
#include <sanitizer/asan_interface.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "segment_copy.hpp"

using namespace nfec;

namespace {

// A page-aligned buffer, poisoned except where a test opens it.  A case uses (fills, opens and
// compares) its first `use` bytes; the rest stays poisoned throughout.
struct Arena {
    uint8_t* p;
    size_t n, use = 0;
    explicit Arena(size_t bytes) : n((bytes + 4095) & ~(size_t)4095)
    {
        p = static_cast<uint8_t*>(aligned_alloc(4096, n));
        if (!p) abort();
    }
    ~Arena()
    {
        __asan_unpoison_memory_region(p, n);
        free(p);
    }
    void fill(uint32_t seed, size_t bytes)
    {
        if (bytes > n) abort();
        use = bytes;
        open_all();
        for (size_t i = 0; i < use; ++i) p[i] = (uint8_t)((((i + seed) * 2654435761u) >> 24) | 1u);  // never zero
    }
    void close() { __asan_poison_memory_region(p, n); }
    void open(const uint8_t* at, size_t bytes) { __asan_unpoison_memory_region(at, bytes); }
    void open_all() { __asan_unpoison_memory_region(p, use); }
};

int failures = 0;
void fail(const char* what, uint32_t len, uint32_t res, uint32_t extra, size_t at)
{
    if (failures++ < 20) std::printf("%s: len %u residue %u (%u): byte %zu\n", what, len, res, extra, at);
}

std::vector<uint32_t> lengths()
{
    std::vector<uint32_t> v;
    for (uint32_t l = 0; l <= 64; ++l) v.push_back(l);
    for (uint32_t l : {1399u, 1400u, 1459u, 1460u}) v.push_back(l);
    return v;
}

constexpr uint32_t kMaxVec = 1460;
constexpr uint32_t kGarbage = 0xdeadbeefu;  // what a lane gets from a neighbour that holds nothing

// ---- gather ----

// the aligned 16-byte chunks that hold a byte of [src, src + len)
void open_source(Arena& a, const uint8_t* src, uint32_t len)
{
    if (!len) return;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(src) & ~(uintptr_t)15;
    const uintptr_t hi = (reinterpret_cast<uintptr_t>(src) + len + 15) & ~(uintptr_t)15;
    a.open(reinterpret_cast<const uint8_t*>(lo), hi - lo);
}

// after a run: the slots hold the sources, zeros to vec, and every other byte of `dst` what `before` holds
void check_gather(const char* what, const Arena& dst, const std::vector<uint8_t>& before,
                  const std::vector<const uint8_t*>& src, const std::vector<uint8_t*>& slot, uint32_t len, uint32_t vec,
                  uint32_t res)
{
    std::vector<uint8_t> want(before);
    for (size_t s = 0; s < slot.size(); ++s) {
        uint8_t* w = want.data() + (slot[s] - dst.p);
        std::memcpy(w, src[s], len);
        std::memset(w + len, 0, vec - len);
    }
    for (size_t i = 0; i < dst.use; ++i)
        if (dst.p[i] != want[i]) return fail(what, len, res, vec, i);
}

void gather_cases()
{
    Arena src(64 * (kMaxVec + 96) + 4096), dst(64 * (kMaxVec + 96) + 4096);
    for (uint32_t len : lengths())
        for (uint32_t sres = 0; sres < 16; ++sres)
            for (uint32_t extra : {0u, 1u, 7u, 9u})
                for (uint32_t dres : {0u, 8u}) {
                    const uint32_t vec = len + extra < kMaxVec ? len + extra : kMaxVec;
                    const uint32_t pieces = gather_pieces(vec);
                    // one source per wave: the lane loop of place_segment
                    {
                        src.fill(len + sres, 64 + 16 + len + 64), dst.fill(vec + dres, 64 + 8 + vec + 64);
                        const uint8_t* s = src.p + 64 + sres;
                        uint8_t* d = dst.p + 64 + dres;
                        const std::vector<uint8_t> before(dst.p, dst.p + dst.use);
                        src.close(), dst.close();
                        open_source(src, s, len);
                        dst.open(d, vec);
                        for (uint32_t lane = 0; lane < 64; ++lane)
                            for (uint32_t p = lane; p < pieces; p += 64) gather_piece(d, s, len, vec, p, PickUniform());
                        src.open_all(), dst.open_all();
                        check_gather("gather, lane loop", dst, before, {s}, {d}, len, vec, sres);
                    }
                    if (!pieces) continue;
                    // a run of segments under one flat index: obj_read_kernel's walk.  Segment sl
                    // starts sl * len bytes further into its 16-byte step, as in an object, but has
                    // a stretch of the arena to itself, so a load that leaves its chunks is caught.
                    {
                        const uint32_t nseg = std::min(std::max(130u / pieces + 1u, 3u), 64u);  // past one wave where it can
                        const uint32_t sstride = (len + 15u + 48u) & ~15u, dstride = ((vec + 7u) & ~7u) + 24u;
                        src.fill(len + sres + 1, 64 + (size_t)nseg * sstride + 64), dst.fill(vec + dres + 1, 64 + 8 + (size_t)nseg * dstride + 64);
                        std::vector<const uint8_t*> s(nseg);
                        std::vector<uint8_t*> d(nseg);
                        for (uint32_t sl = 0; sl < nseg; ++sl) {
                            s[sl] = src.p + 64 + (size_t)sl * sstride + ((sres + sl * len) & 15u);
                            d[sl] = dst.p + 64 + dres + (size_t)sl * dstride;
                        }
                        const std::vector<uint8_t> before(dst.p, dst.p + dst.use);
                        src.close(), dst.close();
                        for (uint32_t sl = 0; sl < nseg; ++sl) open_source(src, s[sl], len), dst.open(d[sl], vec);
                        for (uint32_t f0 = 0; f0 < nseg * pieces; f0 += 64) {  // one wave, one round
                            u32x4 q0[64];
                            bool active[64];
                            for (uint32_t lane = 0; lane < 64; ++lane) {
                                const uint32_t f = f0 + lane, sl = f / pieces, p = f % pieces;
                                active[lane] = sl < nseg;
                                q0[lane] = active[lane] ? gather_first_chunk(s[sl], len, p)
                                                        : u32x4{kGarbage, kGarbage, kGarbage, kGarbage};
                            }
                            for (uint32_t lane = 0; lane < 64; ++lane) {
                                if (!active[lane]) continue;
                                const uint32_t f = f0 + lane, sl = f / pieces, p = f % pieces;
                                const u32x4 next = lane < 63 && active[lane + 1] ? q0[lane + 1]
                                                                                : u32x4{kGarbage, kGarbage, kGarbage, kGarbage};
                                gather_store_piece(d[sl], s[sl], len, vec, p, q0[lane], next,
                                                   gather_second_from_next(lane, p, pieces, len), PickPerLane());
                            }
                        }
                        src.open_all(), dst.open_all();
                        check_gather("gather, flat index", dst, before, s, d, len, vec, sres);
                    }
                }
}

// ---- scatter ----

void scatter_cases()
{
    Arena slot(kMaxVec + 4096), dst(kMaxVec + 4096);
    const uint64_t id = 0xa1b2c3d4e5f60718ull;
    for (uint32_t len : lengths())
        for (uint32_t idlen : {0u, 4u, 8u})
            for (uint32_t dres = 0; dres < 16; ++dres)
                for (uint32_t sres : {0u, 8u})
                    for (uint32_t round = 0; round < 2; ++round) {  // two fillings: what dst held does not matter
                        const uint32_t total = idlen + len;
                        slot.fill(len + sres, 64 + 8 + len + 64), dst.fill(dres + 77u * round, 64 + 16 + total + 64);
                        const uint8_t* s = slot.p + 64 + sres;
                        uint8_t* d = dst.p + 64 + dres;
                        std::vector<uint8_t> want(dst.p, dst.p + dst.use);
                        for (uint32_t j = 0; j < idlen; ++j) want[64 + dres + j] = (uint8_t)(id >> (8 * j));
                        std::memcpy(want.data() + 64 + dres + idlen, s, len);
                        slot.close(), dst.close();
                        slot.open(s, (len + 7u) & ~7u);
                        dst.open(d, total);
                        // emit_message's lane loop; two pieces more, as obj_write_kernel's lanes ask
                        // for pieces a short segment does not have
                        const uint32_t pieces = scatter_pieces(d, total);
                        for (uint32_t lane = 0; lane < 64; ++lane)
                            for (uint32_t p = lane; p < pieces + 2; p += 64) scatter_piece(d, s, len, id, idlen, p);
                        slot.open_all(), dst.open_all();
                        for (size_t i = 0; i < dst.use; ++i)
                            if (dst.p[i] != want[i]) {
                                fail("scatter", len, dres, idlen, i);
                                break;
                            }
                    }
}

}  // namespace

int main()
{
    gather_cases();
    scatter_cases();
    if (failures) {
        std::printf("%d cases failed\n", failures);
        return 1;
    }
    std::printf("segment copy driver done\n");
    return 0;
}
