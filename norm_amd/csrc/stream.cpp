// stream.cpp -- framing a NORM stream object's writes into segments, on the host (no GPU, no codec).
//
// NormStreamObject::Write's loop (reference src/common/normObject.cpp:4039-4232, the body that
// matters :4166-4210) in the closed form of stream_layout.hpp, which the kernels of
// kernels_stream.hip share: the scans are loops here and tiled scans there, the arithmetic per
// element is the same functions.
#include <new>
#include <vector>

#include "nfec_internal.hpp"
#include "stream_layout.hpp"

using namespace nfec;

namespace nfec {

int check_stream_frame(uint32_t segment_size, const nfec_stream_state* state)
{
    if (segment_size < 1 || segment_size > 65535u - kStreamHeader)
        return fail(NFEC_EINVAL, "stream_frame: segment_size outside [1, 65535 - 8]");
    if (state->carry_bytes >= segment_size) return fail(NFEC_EINVAL, "stream_frame: state->carry_bytes >= segment_size");
    if (state->carry_msg_start > state->carry_bytes)
        return fail(NFEC_EINVAL, "stream_frame: state->carry_msg_start > state->carry_bytes");
    return NFEC_OK;
}

}  // namespace nfec

extern "C" int nfec_stream_frame_host(uint32_t segment_size, const uint32_t* write_len, const uint8_t* write_flags,
                                      uint32_t n, nfec_stream_state* state, uint64_t* seg_start, uint16_t* seg_len,
                                      uint16_t* seg_msg_start, uint32_t capacity, uint64_t* totals)
{
    if (!state || !totals) return fail(NFEC_EINVAL, "stream_frame_host: null state or totals");
    if (n && (!write_len || !write_flags)) return fail(NFEC_EINVAL, "stream_frame_host: null write arrays");
    if (capacity && (!seg_start || !seg_len || !seg_msg_start)) return fail(NFEC_EINVAL, "stream_frame_host: null output array");
    int rc = check_stream_frame(segment_size, state);
    if (rc) return rc;
    const uint32_t S = segment_size;
    const bool pending0 = state->msg_start_pending != 0;
    const uint64_t ne = (uint64_t)n + 1u;  // elements: the carry, then the writes
    // per element: first byte, first segment start, own message-start position
    std::vector<uint64_t> B, X0, P, NF, NM;
    try {
        B.resize(ne), X0.resize(ne), P.resize(ne), NF.resize(ne), NM.resize(ne);
    } catch (const std::bad_alloc&) {
        return fail(NFEC_ENOMEM, "stream_frame_host: out of memory");
    }
    auto len_of = [&](uint64_t e) { return e == 0 ? state->carry_bytes : write_len[e - 1]; };
    auto flags_of = [&](uint64_t e) { return e == 0 ? 0u : (uint32_t)write_flags[e - 1]; };
    // the scans over the elements before
    uint64_t pos = 0, G = 0, LN = 0, LE = 0;
    for (uint64_t e = 0; e < ne; ++e) {
        const uint32_t len = len_of(e), fl = flags_of(e);
        B[e] = pos;
        X0[e] = stream_first_start(pos, G, S);
        if (e == 0) P[e] = state->carry_msg_start ? state->carry_msg_start - 1u : kStreamNone;
        else P[e] = stream_is_message_start(len, LN, LE, pending0) ? pos : kStreamNone;
        pos += len;
        if (fl & NFEC_STREAM_FLUSH) G = pos;
        if (e && len) LN = e;
        if (fl & NFEC_STREAM_EOM) LE = e;
    }
    const uint64_t end = pos, consumed = stream_consumed(G, end, S);
    const bool pending1 = stream_flag_raised(LN, LE, pending0);
    // the scans over the elements behind, and the carry's message start
    uint64_t nf = kStreamNone, nm = kStreamNone, carry_p = kStreamNone;
    for (uint64_t e = ne; e-- > 0;) {
        if (flags_of(e) & NFEC_STREAM_FLUSH) nf = B[e] + len_of(e);
        NF[e] = nf, NM[e] = nm;
        if (P[e] != kStreamNone) {
            nm = P[e];
            if (P[e] >= consumed) carry_p = P[e];
        }
    }
    // the segments, element by element
    uint64_t at = 0;
    for (uint64_t e = 0; e < ne; ++e) {
        const uint64_t cnt = stream_closed_count(X0[e], B[e] + len_of(e), NF[e], consumed, S);
        const uint64_t m_first = P[e] != kStreamNone && P[e] >= X0[e] ? P[e] : NM[e];
        for (uint64_t t = 0; t < cnt && at + t < capacity; ++t)
            stream_segment_at(X0[e], t, S, NF[e], m_first, NM[e], seg_start + at + t, seg_len + at + t,
                              seg_msg_start + at + t);
        at += cnt;
    }
    totals[0] = at;
    totals[1] = consumed;
    totals[2] = end - consumed;
    totals[3] = stream_carry_msg_start(carry_p, consumed);
    state->write_offset += (uint32_t)consumed;
    state->msg_start_pending = pending1;
    state->carry_bytes = (uint32_t)totals[2];
    state->carry_msg_start = (uint32_t)totals[3];
    state->next_slot += at;
    return NFEC_OK;
}
