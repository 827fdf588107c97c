// stream_copy_asan.cpp -- the per-segment walks of nfec_stream_pack and nfec_stream_unpack
// (norm_amd/csrc/kernels_stream.hip) as host code, under AddressSanitizer and UBSan, with every
// byte a call may not touch poisoned.  The walks are the kernels': a first wave that fetches and
// judges a run's descriptors (the table entry / the slot's header, by stream_layout.hpp's rules),
// then 256 lanes striding over the run's (segment, 16-byte piece) pairs as one flat index with
// segment_copy.hpp's gather / scatter on the slot's bytes from 8 on.  What is checked is what
// nfec.h promises of a wrong table and of a header off the network: a slot that ends its
// allocation, a stream buffer and a window that end theirs, and entries and headers that claim
// too much touch nothing outside.  Host code only, no GPU; `make -C tests/native -f
// stream_copy_asan.mk`.
//
// ASan poisons whole 8-byte granules or their tails, so the bytes between a destination's granule
// and an unaligned first byte stay addressable; a store there is caught by comparing every byte
// with what it has to hold.
#include <sanitizer/asan_interface.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "segment_copy.hpp"
#include "stream_layout.hpp"

using namespace nfec;

namespace {

// A page-aligned buffer whose last byte is the allocation's last: what lies behind it is the
// allocator's red zone.  A case uses the last `bytes` of it.
struct Arena {
    uint8_t* p;
    size_t n;
    explicit Arena(size_t bytes) : n((bytes + 4095) & ~(size_t)4095)
    {
        p = static_cast<uint8_t*>(aligned_alloc(4096, n));
        if (!p) abort();
    }
    ~Arena()
    {
        open_all();
        free(p);
    }
    uint8_t* end() const { return p + n; }
    void fill(uint32_t seed)
    {
        open_all();
        for (size_t i = 0; i < n; ++i) p[i] = (uint8_t)((((i + seed) * 2654435761u) >> 24) | 1u);  // never zero
    }
    void close() { __asan_poison_memory_region(p, n); }
    void open(const uint8_t* at, size_t bytes) { __asan_unpoison_memory_region(at, bytes); }
    void open_all() { __asan_unpoison_memory_region(p, n); }
};

int failures = 0;
void fail(const char* what, uint32_t S, uint32_t res, size_t at)
{
    if (failures++ < 20) std::printf("%s: segment_size %u residue %u: byte %zu\n", what, S, res, at);
}

constexpr uint32_t kRun = 64;
constexpr uint32_t kSkip = ~0u;
constexpr uint32_t kGarbage = 0xdeadbeefu;  // what a lane gets from a neighbour that holds nothing

uint32_t length_of(uint32_t n, uint32_t S)
{
    const uint32_t pick[4] = {1u, S > 1 ? S - 1u : 1u, S, 1u + (n * 7919u) % S};
    return pick[n % 4];
}

// ---- pack ----

// One run of stream_pack_kernel: nseg slots from `slot0` on, entry i of the table for slot i.
void pack_run(uint8_t* slot0, uint32_t seg_stride, uint32_t vec, uint32_t nseg, const uint8_t* bytes, uint64_t stream_bytes,
              const std::vector<uint64_t>& start, const std::vector<uint16_t>& len, const std::vector<uint16_t>& ms,
              uint32_t S, uint32_t write_offset)
{
    uint64_t s_src[kRun];
    uint32_t s_len[kRun];
    for (uint32_t tid = 0; tid < kRun; ++tid) {  // the first wave
        uint64_t st = 0;
        uint32_t ln = kSkip;
        if (tid < nseg && stream_entry_ok(start[tid], len[tid], S, stream_bytes)) {
            st = start[tid], ln = len[tid];
            uint32_t w0, w1;
            stream_header_encode(ln, ms[tid], write_offset + (uint32_t)st, &w0, &w1);
            *reinterpret_cast<u32x2*>(slot0 + (size_t)tid * seg_stride) = u32x2{w0, w1};
        }
        s_src[tid] = st, s_len[tid] = ln;
    }
    const uint32_t pieces = gather_pieces(vec - kStreamHeader);
    for (uint32_t f0 = 0; f0 < nseg * pieces; f0 += 64) {  // one wave, one round
        u32x4 c0[64];
        bool active[64];
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t f = f0 + lane, sl = f / pieces, p = f % pieces;
            active[lane] = sl < nseg;
            c0[lane] = u32x4{kGarbage, kGarbage, kGarbage, kGarbage};
            if (active[lane]) c0[lane] = gather_first_chunk(bytes + s_src[sl], s_len[sl] == kSkip ? 0u : s_len[sl], p);
        }
        for (uint32_t lane = 0; lane < 64; ++lane) {
            if (!active[lane]) continue;
            const uint32_t f = f0 + lane, sl = f / pieces, p = f % pieces;
            if (s_len[sl] == kSkip) continue;
            const u32x4 next = lane < 63 && active[lane + 1] ? c0[lane + 1] : u32x4{kGarbage, kGarbage, kGarbage, kGarbage};
            gather_store_piece(slot0 + (size_t)sl * seg_stride + kStreamHeader, bytes + s_src[sl], s_len[sl],
                               vec - kStreamHeader, p, c0[lane], next, gather_second_from_next(lane, p, pieces, s_len[sl]),
                               PickPerLane());
        }
    }
}

void pack_cases()
{
    for (uint32_t S : {1u, 2u, 37u, 48u, 1392u, 1452u})
        for (uint32_t extra : {0u, 5u})
            for (uint32_t sres = 0; sres < 16; ++sres) {
                const uint32_t vec = S + kStreamHeader + extra, seg_stride = (vec + 7u) & ~7u;
                const uint32_t nseg = S > 100 ? 9u : 64u;
                // the table: segments one behind the other, the last ending the stream bytes
                std::vector<uint64_t> start(nseg);
                std::vector<uint16_t> len(nseg), ms(nseg);
                uint64_t at = 0;
                for (uint32_t i = 0; i < nseg; ++i) {
                    start[i] = at, len[i] = (uint16_t)length_of(i + sres, S), ms[i] = (uint16_t)(i % 3 ? 0 : 1 + i % len[i]);
                    at += len[i];
                }
                const uint64_t stream_bytes = at;
                // entries that claim too much: too long, empty, past the end by one byte, far past it
                std::vector<bool> bad(nseg, false);
                const uint32_t b0 = 1, b1 = 3, b2 = nseg - 2, b3 = 5;
                len[b0] = (uint16_t)(S + 1u), len[b1] = 0, start[b2] = stream_bytes - len[b2] + 1u, start[b3] = ~0ull - 3u;
                bad[b0] = bad[b1] = bad[b2] = bad[b3] = true;
                // the stream bytes end their allocation, at residue sres from a 16-byte boundary
                // before them; the slots end theirs
                Arena src(stream_bytes + 64), dst((size_t)nseg * seg_stride);
                src.fill(S + sres), dst.fill(vec + sres);
                const size_t pad = (16u - (sres + stream_bytes) % 16u) % 16u;  // so that bytes % 16 == sres
                // (the allocation's end is 16-byte aligned: move the stream's end back by `pad`, and
                // keep what lies behind it poisoned as if the allocation ended there)
                const uint8_t* bytes = src.end() - pad - stream_bytes;
                if ((reinterpret_cast<uintptr_t>(bytes) & 15u) != sres) abort();
                uint8_t* slot0 = dst.end() - (size_t)nseg * seg_stride;
                std::vector<uint8_t> want(dst.p, dst.end());
                const uint32_t write_offset = 0xfffffff0u;
                for (uint32_t i = 0; i < nseg; ++i) {
                    if (bad[i]) continue;
                    uint8_t* w = want.data() + (slot0 - dst.p) + (size_t)i * seg_stride;
                    const uint32_t off = write_offset + (uint32_t)start[i];
                    const uint8_t h[8] = {(uint8_t)(len[i] >> 8), (uint8_t)len[i], (uint8_t)(ms[i] >> 8), (uint8_t)ms[i],
                                          (uint8_t)(off >> 24), (uint8_t)(off >> 16), (uint8_t)(off >> 8), (uint8_t)off};
                    std::memcpy(w, h, 8);
                    std::memcpy(w + 8, bytes + start[i], len[i]);
                    std::memset(w + 8 + len[i], 0, vec - 8u - len[i]);
                }
                src.close(), dst.close();
                for (uint32_t i = 0; i < nseg; ++i) {
                    if (bad[i]) continue;  // a rejected entry's slot and bytes stay closed
                    const uintptr_t lo = reinterpret_cast<uintptr_t>(bytes + start[i]) & ~(uintptr_t)15;
                    const uintptr_t hi = (reinterpret_cast<uintptr_t>(bytes + start[i]) + len[i] + 15) & ~(uintptr_t)15;
                    src.open(reinterpret_cast<const uint8_t*>(lo), std::min<uintptr_t>(hi, reinterpret_cast<uintptr_t>(src.end())) - lo);
                    dst.open(slot0 + (size_t)i * seg_stride, vec);
                }
                pack_run(slot0, seg_stride, vec, nseg, bytes, stream_bytes, start, len, ms, S, write_offset);
                src.open_all(), dst.open_all();
                for (size_t i = 0; i < dst.n; ++i)
                    if (dst.p[i] != want[i]) {
                        fail("pack", S, sres, i);
                        break;
                    }
            }
}

// ---- unpack ----

// One run of stream_unpack_kernel: every slot selected.
void unpack_run(const uint8_t* slot0, uint32_t seg_stride, uint32_t nseg, uint8_t* window, uint64_t window_bytes,
                uint32_t base_offset, uint32_t S, uint32_t* counts)
{
    uint32_t s_dst[kRun], s_len[kRun];
    for (uint32_t tid = 0; tid < kRun; ++tid) {  // the first wave
        s_dst[tid] = 0, s_len[tid] = 0;
        if (tid >= nseg) continue;
        const u32x2 h = *reinterpret_cast<const u32x2*>(slot0 + (size_t)tid * seg_stride);
        uint32_t len, ms, off, d;
        stream_header_decode(h[0], h[1], &len, &ms, &off);
        const uint32_t verdict = stream_header_verdict(len, off, base_offset, S, window_bytes, &d);
        ++counts[verdict];
        s_dst[tid] = d, s_len[tid] = verdict == STREAM_DELIVER ? len : 0u;
    }
    const uint32_t pieces = (S + 30u) / 16u;
    for (uint32_t f = 0; f < nseg * pieces; ++f) {
        const uint32_t sl = f / pieces, p = f % pieces;
        if (!s_len[sl]) continue;
        scatter_piece(window + s_dst[sl], slot0 + (size_t)sl * seg_stride + kStreamHeader, s_len[sl], 0, 0, p);
    }
}

void put_header(uint8_t* slot, uint32_t len, uint32_t ms, uint32_t off)
{
    const uint8_t h[8] = {(uint8_t)(len >> 8), (uint8_t)len, (uint8_t)(ms >> 8), (uint8_t)ms,
                          (uint8_t)(off >> 24), (uint8_t)(off >> 16), (uint8_t)(off >> 8), (uint8_t)off};
    std::memcpy(slot, h, 8);
}

void unpack_cases()
{
    for (uint32_t S : {1u, 2u, 37u, 48u, 1392u, 1452u})
        for (uint32_t extra : {0u, 5u})
            for (uint32_t wres = 0; wres < 16; ++wres) {
                const uint32_t vec = S + kStreamHeader + extra, seg_stride = (vec + 7u) & ~7u;
                const uint32_t nseg = S > 100 ? 12u : 64u;
                const uint32_t base_offset = 0xffffff00u + wres;  // the offsets wrap inside the window
                // good segments tile the window, whose last byte ends its allocation
                std::vector<uint32_t> len(nseg), d(nseg);
                std::vector<int> kind(nseg, 0);  // 0 deliver, 2 control, 3 invalid
                uint32_t at = 0;
                for (uint32_t i = 0; i < nseg; ++i) {
                    len[i] = length_of(i + wres, S), d[i] = at;
                    if (i % 6 == 1 || i + 1 == nseg) kind[i] = i % 4 == 1 ? 2 : 3;
                    else at += len[i];
                }
                const uint64_t window_bytes = at;
                Arena slots((size_t)nseg * seg_stride), win(window_bytes + 64 + wres);
                slots.fill(S + wres), win.fill(vec + wres);
                uint8_t* slot0 = slots.end() - (size_t)nseg * seg_stride;
                // (at residue wres: the window's end moves back from the allocation's by `tail` bytes,
                // which stay poisoned as if the allocation ended there)
                const size_t tail = (16u - (wres + window_bytes) % 16u) % 16u;
                uint8_t* window = win.end() - tail - window_bytes;
                std::vector<uint8_t> want(win.p, win.end());
                uint32_t bad = 0, expect[4] = {0, 0, 0, 0};
                for (uint32_t i = 0; i < nseg; ++i) {
                    uint8_t* slot = slot0 + (size_t)i * seg_stride;
                    uint32_t off = base_offset + d[i], ln = len[i];
                    if (kind[i] == 2) ln = 0;
                    if (kind[i] == 3) {
                        // headers that claim too much: a length past the segment size or the slot, an
                        // offset before the window, one that ends a byte past it, one 2^31 away
                        switch (bad++ % 5) {
                        case 0: ln = S + 1u; break;
                        case 1: ln = 0xffffu; break;
                        case 2: off = base_offset - 1u; break;
                        case 3: off = base_offset + (uint32_t)window_bytes - ln + 1u; break;
                        default: off = base_offset + 0x80000000u; break;
                        }
                    }
                    put_header(slot, ln, i % 2 ? 0u : 1u, off);
                    ++expect[kind[i]];
                    if (kind[i] == 0) std::memcpy(want.data() + (window - win.p) + d[i], slot + 8, ln);
                }
                slots.close(), win.close();
                for (uint32_t i = 0; i < nseg; ++i) {
                    // the header, and for a segment that is delivered the 8-byte chunks of its bytes
                    slots.open(slot0 + (size_t)i * seg_stride, kind[i] == 0 ? 8u + ((len[i] + 7u) & ~7u) : 8u);
                    if (kind[i] == 0) win.open(window + d[i], len[i]);
                }
                uint32_t counts[4] = {0, 0, 0, 0};
                unpack_run(slot0, seg_stride, nseg, window, window_bytes, base_offset, S, counts);
                slots.open_all(), win.open_all();
                for (size_t i = 0; i < win.n; ++i)
                    if (win.p[i] != want[i]) {
                        fail("unpack", S, wres, i);
                        break;
                    }
                if (std::memcmp(counts, expect, sizeof(counts)) != 0 || !expect[0] || !expect[3]) fail("unpack counts", S, wres, 0);
            }
}

}  // namespace

int main()
{
    pack_cases();
    unpack_cases();
    if (failures) {
        std::printf("%d cases failed\n", failures);
        return 1;
    }
    std::printf("stream copy driver done\n");
    return 0;
}
