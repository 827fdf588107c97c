// segment_copy.hpp -- the two misaligned-copy rules of the device sender, receiver and object paths,
// one 16-byte piece at a time.  Shared by the kernels (kernels_rx.hip, kernels_tx.hip,
// kernels_obj.hip, kernels_stream.hip, kernels_datamsg.hip) and host drivers
// (tests/native/segment_copy_asan.cpp; data_msg_asan.cpp for the header form) that run the same
// arithmetic under AddressSanitizer with everything outside the permitted bytes unaddressable: what
// the comments below claim about loads and stores is what that driver checks.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NFEC_SC_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define NFEC_SC_HD inline
#endif

namespace nfec {

typedef uint32_t u32x4 __attribute__((vector_size(16)));
typedef uint32_t u32x2 __attribute__((vector_size(8)));

// v_alignbyte_b32: bytes [sh, sh + 4) of the eight bytes hi:lo (sh 0..3)
NFEC_SC_HD uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t sh)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * (sh & 3u)));
#endif
}

// the low n bytes of a dword (n <= 0: none, n >= 4: all)
NFEC_SC_HD uint32_t low_bytes(int32_t n) { return n >= 4 ? ~0u : n <= 0 ? 0u : (1u << (8 * n)) - 1u; }

// ---- gather: an unaligned source into an 8-byte aligned slot, zero-padded to vec ----
//
// Piece p of a slot is its bytes [16p, 16p + 16), for p < gather_pieces(vec).  They are the source
// bytes src[16p ...], src at any alignment, up to the source's `len` bytes, and zeros from `len` to
// `vec` (the reference's zero pad of a short segment).  With sh = src mod 16 = 4 dsh + bsh the
// piece lies in the two aligned 16-byte chunks p and p + 1 counted from src - sh: dsh picks five
// of their eight dwords (the caller says how, below) and the byte funnel shifts them by bsh.  A chunk is loaded only when it
// holds a source byte the piece needs -- the first when the source reaches the piece, the second
// when, besides, src is misaligned and the source reaches past the first -- so every load is of an
// aligned chunk that holds a byte of [src, src + len): no load leaves a page the source touches,
// and a source of no bytes is not read.  A whole piece is stored as one 16-byte store where the
// slot is 16-byte aligned and as two 8-byte stores elsewhere; the piece that holds byte `vec` is
// stored by bytes (behind one 8-byte store where 8 bytes are the vector's), so nothing outside
// [slot, slot + vec) is stored and the stride padding past `vec` keeps the caller's bytes.  The
// slot is never read.
//
// The second chunk of piece p is the first chunk of piece p + 1.  A caller whose neighbouring lane
// holds that piece of the same source passes it in (`next_q0`) instead of loading it twice:
// gather_second_from_next says when the neighbour has it.

NFEC_SC_HD uint32_t gather_pieces(uint32_t vec) { return (vec + 15u) / 16u; }

// source bytes from the piece's first byte on (may be <= 0 or > 16)
NFEC_SC_HD int32_t gather_valid(uint32_t len, uint32_t p) { return (int32_t)len - (int32_t)(16u * p); }

// the piece's first chunk, or zeros where the source ends before the piece
NFEC_SC_HD u32x4 gather_first_chunk(const uint8_t* __restrict__ src, uint32_t len, uint32_t p)
{
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u);
    u32x4 q0 = {0u, 0u, 0u, 0u};
    if (gather_valid(len, p) > 0) q0 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src - sh) + p);
    return q0;
}

// The lane after `lane` holds piece p + 1 of the same source (the caller's lanes take consecutive
// pieces, `pieces` per source) and has loaded its first chunk: the source reaches past piece p.
NFEC_SC_HD bool gather_second_from_next(uint32_t lane, uint32_t p, uint32_t pieces, uint32_t len)
{
    return lane != 63u && p + 1u < pieces && gather_valid(len, p) > 16;
}

// The dword pick: dwords dsh .. dsh + 4 of the eight in q0, q1.  The one step of the rule with two
// forms, because what is cheap depends on whether dsh differs between the lanes of a wave; the
// caller of gather_store_piece passes the one that fits its lanes.  Both are correct for any lanes.
struct PickPerLane {  // by two dwords, then by one: selects, no branch
    NFEC_SC_HD void operator()(uint32_t dsh, u32x4 q0, u32x4 q1, uint32_t (&e)[5]) const
    {
        const bool by2 = dsh & 2u, by1 = dsh & 1u;
        const uint32_t t0 = by2 ? q0[2] : q0[0], t1 = by2 ? q0[3] : q0[1], t2 = by2 ? q1[0] : q0[2],
                       t3 = by2 ? q1[1] : q0[3], t4 = by2 ? q1[2] : q1[0], t5 = by2 ? q1[3] : q1[1];
        e[0] = by1 ? t1 : t0, e[1] = by1 ? t2 : t1, e[2] = by1 ? t3 : t2, e[3] = by1 ? t4 : t3, e[4] = by1 ? t5 : t4;
    }
};
struct PickUniform {  // a branch, which is a scalar one where dsh is wave-uniform
    NFEC_SC_HD void operator()(uint32_t dsh, u32x4 q0, u32x4 q1, uint32_t (&e)[5]) const
    {
        switch (dsh) {
        case 0: e[0] = q0[0], e[1] = q0[1], e[2] = q0[2], e[3] = q0[3], e[4] = q1[0]; break;
        case 1: e[0] = q0[1], e[1] = q0[2], e[2] = q0[3], e[3] = q1[0], e[4] = q1[1]; break;
        case 2: e[0] = q0[2], e[1] = q0[3], e[2] = q1[0], e[3] = q1[1], e[4] = q1[2]; break;
        default: e[0] = q0[3], e[1] = q1[0], e[2] = q1[1], e[3] = q1[2], e[4] = q1[3]; break;
        }
    }
};

// Piece p from its first chunk q0 (gather_first_chunk).  from_next: next_q0 is the second chunk;
// otherwise it is loaded here when the piece needs it, and next_q0 may hold anything.
template <typename Pick>
NFEC_SC_HD void gather_store_piece(uint8_t* __restrict__ slot, const uint8_t* __restrict__ src, uint32_t len, uint32_t vec,
                                   uint32_t p, u32x4 q0, u32x4 next_q0, bool from_next, Pick pick)
{
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u);
    const uint32_t dsh = sh >> 2, bsh = sh & 3u;
    const int32_t nvalid = gather_valid(len, p);
    u32x4 q1 = next_q0;
    if (nvalid > 0 && sh != 0 && (int32_t)sh + nvalid > 16 && !from_next)
        q1 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src - sh) + p + 1);
    // (Where no second chunk was needed q1 is arbitrary: with sh == 0 none of it is picked,
    // otherwise the source ends inside q0 and the mask below clears what follows.)
    uint32_t e[5];
    pick(dsh, q0, q1, e);
    uint32_t o[4] = {alignbyte(e[1], e[0], bsh), alignbyte(e[2], e[1], bsh), alignbyte(e[3], e[2], bsh),
                     alignbyte(e[4], e[3], bsh)};
    if (nvalid < 16) {  // the source ends inside or before the piece: zeros from there on
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] &= low_bytes(nvalid - 4 * j);
    }
    const uint32_t nw = vec - 16u * p;  // bytes of this piece inside the vector (> 0; >= 16: all)
    uint8_t* d = slot + 16u * p;
    if (nw >= 16) {
        if ((reinterpret_cast<uintptr_t>(d) & 15u) == 0) {  // (the slot's own residue: uniform where the slot is)
            *reinterpret_cast<u32x4*>(d) = u32x4{o[0], o[1], o[2], o[3]};
        } else {
            *reinterpret_cast<u32x2*>(d) = u32x2{o[0], o[1]};
            *reinterpret_cast<u32x2*>(d + 8) = u32x2{o[2], o[3]};
        }
    } else {
        uint32_t lo = o[0], hi = o[1], done = 0;
        if (nw >= 8) {
            *reinterpret_cast<u32x2*>(d) = u32x2{o[0], o[1]};
            lo = o[2], hi = o[3], done = 8;
        }
        const uint64_t v = ((uint64_t)hi << 32) | lo;
        for (uint32_t t = done; t < nw; ++t) d[t] = (uint8_t)(v >> (8 * (t - done)));
    }
}

// piece p with both chunks loaded here
template <typename Pick>
NFEC_SC_HD void gather_piece(uint8_t* __restrict__ slot, const uint8_t* __restrict__ src, uint32_t len, uint32_t vec,
                             uint32_t p, Pick pick)
{
    gather_store_piece(slot, src, len, vec, p, gather_first_chunk(src, len, p), u32x4{0u, 0u, 0u, 0u}, false, pick);
}

// ---- scatter: an 8-byte aligned slot to any byte address, behind an optional payload ID ----
//
// The message is `idlen` bytes of ID (byte j of it is bits [8j, 8j + 8) of `id`; idlen <= 8) and
// the slot's first `len` bytes; it goes to [dst, dst + idlen + len), dst at any alignment.  The
// destination is cut into the aligned 16-byte pieces that hold it, counted from the piece that
// holds dst[0]: scatter_pieces of them.  A piece's slot bytes start `sh` bytes into a 16-byte step
// of the slot, the same sh for every piece of a message; dsh and the byte funnel bring them into
// place.  Loads are 8-byte chunks of the slot (a slot is 8-byte, not 16-byte, aligned, and it may
// end the allocation): three cover a piece's 16 bytes at any shift, and a chunk is loaded only
// when it holds a slot byte the piece stores, which keeps every load inside [slot, slot + len
// rounded up to 8) and so inside seg_stride.  A piece wholly inside the message is one 16-byte
// store; the first and the last piece store only their own bytes, as dwords where a whole dword is
// theirs and as bytes elsewhere: a neighbouring message or segment, written by another wave at the
// same time, may share the piece, so nothing outside the message is stored, and the destination is
// never read.

NFEC_SC_HD uint32_t scatter_pieces(const uint8_t* dst, uint32_t total)
{
    return total ? ((uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u) + total + 15u) >> 4 : 0u;
}

// The slot's bytes of piece p, in place, for a message whose slot byte 0 lies q bytes into piece 0
// (q = dst mod 16 + the bytes in front of the payload): piece p holds slot bytes [16 (p - pb) + sh,
// + 16).  The bytes of o[] that are not the slot's are zero or arbitrary.
NFEC_SC_HD void scatter_slot_bytes(const uint8_t* __restrict__ slot, uint32_t len, uint32_t q, uint32_t p, uint32_t (&o)[4])
{
    const int32_t pb = (int32_t)((q + 15u) >> 4);
    const uint32_t sh = (0u - q) & 15u;
    const uint32_t dsh = (sh >> 2) & 1u, bsh = sh & 3u;
    const u32x2* __restrict__ chunk = reinterpret_cast<const u32x2*>(slot);
    const int32_t sidx = 16 * ((int32_t)p - pb) + (int32_t)sh;  // the piece's first slot byte (may be < 0)
    const int32_t need_lo = sidx > 0 ? sidx : 0, need_hi = sidx + 16 < (int32_t)len ? sidx + 16 : (int32_t)len;
    const int32_t c0 = 2 * ((int32_t)p - pb) + (int32_t)(sh >> 3);
    uint32_t e[6];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int32_t c = c0 + j;
        u32x2 v = {0u, 0u};
        if (8 * c < need_hi && 8 * c + 8 > need_lo) v = __builtin_nontemporal_load(chunk + c);
        e[2 * j] = v[0], e[2 * j + 1] = v[1];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = alignbyte(dsh ? e[j + 2] : e[j + 1], dsh ? e[j + 1] : e[j], bsh);
}

// Piece p's own bytes of o[] to the destination: all 16 where the message covers the piece, else
// as dwords where a whole dword is the message's and as bytes elsewhere.  total: the message's bytes.
NFEC_SC_HD void scatter_store(uint8_t* __restrict__ dst, uint32_t total, uint32_t p, const uint32_t (&o)[4])
{
    const uint32_t dres = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
    const uint32_t first = p * 16u;  // the piece's first byte, counted from piece 0
    const uint32_t lo = p == 0 ? dres : 0u;
    const uint32_t hi = dres + total - first < 16u ? dres + total - first : 16u;
    uint8_t* d = dst - dres + first;
    if (lo == 0 && hi == 16) {
        *reinterpret_cast<u32x4*>(d) = u32x4{o[0], o[1], o[2], o[3]};
    } else {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t at = 4u * w;
            if (lo <= at && at + 4u <= hi) {
                *reinterpret_cast<uint32_t*>(d + at) = o[w];
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (lo <= at + t && at + t < hi) d[at + t] = (uint8_t)(o[w] >> (8 * t));
            }
        }
    }
}

// piece p of the message; no store when the message has no piece p
NFEC_SC_HD void scatter_piece(uint8_t* __restrict__ dst, const uint8_t* __restrict__ slot, uint32_t len, uint64_t id,
                              uint32_t idlen, uint32_t p)
{
    const uint32_t total = idlen + len;
    if (p >= scatter_pieces(dst, total)) return;
    const uint32_t dres = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
    const uint32_t q = dres + idlen;  // slot byte 0 lies q bytes into piece 0
    uint32_t o[4];
    scatter_slot_bytes(slot, len, q, p, o);
    const uint32_t first = p * 16u;  // the piece's first byte, counted from piece 0
    if (first < q) {
        // the piece may hold ID bytes: byte t of it is message byte first + t - dres
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const uint32_t j = first + 4u * w + t - dres;  // (wraps below the message: j >= idlen)
                if (j < idlen) o[w] = (o[w] & ~(0xffu << (8 * t))) | ((uint32_t)((id >> (8u * j)) & 0xffu) << (8 * t));
            }
    }
    scatter_store(dst, total, p, o);
}

// ---- scatter behind a message header of up to 40 bytes (a NORM_DATA header, data_msg.hpp) ----
//
// The same rule with `hlen` header bytes (a multiple of 4) in front of the payload instead of an
// ID of at most 8.  The header is given as words (byte j of the header in bits [8 (j mod 4), + 8) of
// hdr[j / 4]; words past hlen / 4 are zero), the same for every lane of a wave.  It reaches into
// pieces 0 .. 3 at the most (15 + 40 bytes), so it is first brought to where it lies in those four
// pieces -- img[i] is bytes [4i, 4i + 4) of pieces 0 .. 3, header byte j at byte dst mod 16 + j --
// by one byte funnel and a dword shift that are uniform where dst is, with no indexing by a lane's
// value; a lane then picks its piece's four words of the image by selects.
constexpr uint32_t kScatterHeaderWords = 10;

NFEC_SC_HD void scatter_header_image(const uint32_t (&hdr)[kScatterHeaderWords], uint32_t dres, uint32_t (&img)[16])
{
    const uint32_t ds = dres >> 2, bs = dres & 3u;
    // pre[k]: header bytes [4k - bs, 4k - bs + 4) (zero in front of and behind the header)
    uint32_t pre[kScatterHeaderWords + 1];
#pragma unroll
    for (uint32_t k = 0; k <= kScatterHeaderWords; ++k) {
        const uint32_t cur = k < kScatterHeaderWords ? hdr[k] : 0u, prev = k ? hdr[k - 1] : 0u;
        pre[k] = alignbyte(cur, bs ? prev : cur, (4u - bs) & 3u);
    }
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) img[i] = 0u;
    switch (ds) {
    case 0:
#pragma unroll
        for (uint32_t k = 0; k <= kScatterHeaderWords; ++k) img[k] = pre[k];
        break;
    case 1:
#pragma unroll
        for (uint32_t k = 0; k <= kScatterHeaderWords; ++k) img[k + 1] = pre[k];
        break;
    case 2:
#pragma unroll
        for (uint32_t k = 0; k <= kScatterHeaderWords; ++k) img[k + 2] = pre[k];
        break;
    default:
#pragma unroll
        for (uint32_t k = 0; k <= kScatterHeaderWords; ++k) img[k + 3] = pre[k];
        break;
    }
}

// piece p of the message [dst, dst + hlen + len): the header, then the slot's first len bytes; no
// store when the message has no piece p.  img: scatter_header_image of the header at dst mod 16.
NFEC_SC_HD void scatter_piece_header(uint8_t* __restrict__ dst, const uint8_t* __restrict__ slot, uint32_t len,
                                     const uint32_t (&img)[16], uint32_t hlen, uint32_t p)
{
    const uint32_t total = hlen + len;
    if (p >= scatter_pieces(dst, total)) return;
    const uint32_t dres = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
    const uint32_t q = dres + hlen;  // slot byte 0 lies q bytes into piece 0
    uint32_t o[4];
    scatter_slot_bytes(slot, len, q, p, o);
    const uint32_t first = p * 16u;
    if (first < q) {
        // the piece holds header bytes: those of its bytes that lie below q (p <= 3 here)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t hv = p == 0 ? img[w] : p == 1 ? img[4 + w] : p == 2 ? img[8 + w] : img[12 + w];
            const uint32_t m = low_bytes((int32_t)q - (int32_t)(first + 4u * w));
            o[w] = (o[w] & ~m) | (hv & m);
        }
    }
    scatter_store(dst, total, p, o);
}

}  // namespace nfec
