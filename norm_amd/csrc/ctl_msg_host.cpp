// ctl_msg_host.cpp -- the host twins of the NORM_NACK / REPAIR_ADV message calls (nfec.h, "NORM_NACK
// and NORM_CMD(REPAIR_ADV) messages on the device"): no GPU, no codec.  The header words, the cut
// (cut_message over a request index) and the parse are ctl_msg.hpp's, the code the kernels of
// kernels_ctlmsg.hip run; this file moves bytes in and out of them and holds the argument checks the
// device entries share.
#include "ctl_msg.hpp"
#include "nfec_internal.hpp"

#include <vector>

using namespace nfec;

namespace nfec {

static void ext_words(const uint8_t* ext, uint32_t ext_bytes, uint32_t (&w)[3])
{
    for (uint32_t j = 0; j < 3; ++j) {
        w[j] = 0;
        for (uint32_t t = 0; t < 4; ++t)
            if (4 * j + t < ext_bytes) w[j] |= (uint32_t)ext[4 * j + t] << (8u * t);
    }
}

int nack_header_fixed_from(const nfec_nack_header* h, CtlHeaderFixed& f)
{
    if (!h) return fail(NFEC_EINVAL, "nack header: null header");
    if (h->ext_bytes != 0 && h->ext_bytes != kCtlExtBytes) return fail(NFEC_EINVAL, "nack header: ext_bytes is neither 0 nor 12");
    uint32_t e[3];
    ext_words(h->ext, h->ext_bytes, e);
    nack_header_fixed(f, h->source_id, h->sender_id, h->instance_id, h->grtt_response_sec, h->grtt_response_usec, e, h->ext_bytes);
    f.first_sequence = h->first_sequence;
    f.sequence_step = h->sequence_step;
    return NFEC_OK;
}

int adv_header_fixed_from(const nfec_adv_header* h, CtlHeaderFixed& f)
{
    if (!h) return fail(NFEC_EINVAL, "adv header: null header");
    if (h->ext_bytes != 0 && h->ext_bytes != kCtlExtBytes) return fail(NFEC_EINVAL, "adv header: ext_bytes is neither 0 nor 12");
    if (h->backoff > 15 || h->gsize > 15) return fail(NFEC_EINVAL, "adv header: backoff or gsize above 15");
    uint32_t e[3];
    ext_words(h->ext, h->ext_bytes, e);
    adv_header_fixed(f, h->source_id, h->instance_id, h->sequence, h->grtt, h->backoff, h->gsize, e, h->ext_bytes);
    return NFEC_OK;
}

int ctl_filter_from(const nfec_ctl_filter* in, CtlFilter& f)
{
    if (!in) return fail(NFEC_EINVAL, "ctl filter: null filter");
    if (in->flags & ~(uint32_t)(NFEC_CTL_ANY_INSTANCE | NFEC_CTL_TAKE_NACK | NFEC_CTL_TAKE_ADV))
        return fail(NFEC_EINVAL, "ctl filter: unknown flags");
    f.sender_id = in->sender_id;
    f.instance_id = in->instance_id;
    f.local_id = in->local_id;
    f.flags = in->flags;
    return NFEC_OK;
}

int cut_params_from(uint8_t fec_id, uint32_t segment_size, uint32_t hdr_bytes, CutParams& c, const char* what)
{
    const uint32_t idlen = data_id_length(fec_id);
    if (!idlen) return fail(NFEC_EINVAL, std::string(what) + ": unknown fec_id");
    c.L = 4u + idlen;
    c.S = segment_size;
    if (!cut_params_ok(segment_size, c.L, hdr_bytes))
        return fail(NFEC_EINVAL, std::string(what) + ": segment_size is no multiple of 4, below 4 + 2 item lengths, or "
                                                     "segment_size + header above 65535");
    return NFEC_OK;
}

namespace {

// the content's dwords at any alignment (byte j of a dword in its bits [8j, 8j + 8))
struct HostContent {
    const uint8_t* bytes;
    uint32_t operator()(uint64_t off) const
    {
        return (uint32_t)bytes[off] | ((uint32_t)bytes[off + 1] << 8) | ((uint32_t)bytes[off + 2] << 16) | ((uint32_t)bytes[off + 3] << 24);
    }
};

// the request index of content[0, bytes): the walk's stop is x.end
void index_requests(const HostContent& load, uint64_t bytes, uint32_t L, std::vector<uint32_t>& req, uint64_t* end)
{
    uint64_t off = 0;
    while (off < bytes) {
        CutRequest q;
        if (bytes - off < 4 || !cut_request(load(off), bytes - off - 4, L, q)) break;
        req.push_back((uint32_t)(off / 4));
        off += 4u + q.len;
    }
    *end = off;
}

void put_word(uint8_t* at, uint32_t w)
{
    for (uint32_t t = 0; t < 4; ++t) at[t] = (uint8_t)(w >> (8u * t));
}

// message m's content bytes into out
void put_content(const CutMessage& m, const uint8_t* content, uint8_t* out)
{
    for (uint32_t j = 4; j < m.length; ++j) out[j] = content[m.src + j];
    put_word(out, m.head);
    if (m.tail_at) put_word(out + m.tail_at, m.tail);
}

}  // namespace

}  // namespace nfec

extern "C" int nfec_nack_header_bytes(uint8_t ext_bytes)
{
    if (ext_bytes != 0 && ext_bytes != kCtlExtBytes) return fail(NFEC_EINVAL, "nack_header_bytes: ext_bytes is neither 0 nor 12");
    return (int)(kNackBase + ext_bytes);
}

extern "C" int nfec_adv_header_bytes(uint8_t ext_bytes)
{
    if (ext_bytes != 0 && ext_bytes != kCtlExtBytes) return fail(NFEC_EINVAL, "adv_header_bytes: ext_bytes is neither 0 nor 12");
    return (int)(kAdvBase + ext_bytes);
}

extern "C" int nfec_nack_header_write_host(const nfec_nack_header* header, uint32_t i, void* out, size_t cap)
{
    CtlHeaderFixed f;
    const int rc = nack_header_fixed_from(header, f);
    if (rc) return rc;
    if (!out) return fail(NFEC_EINVAL, "nack_header_write_host: null out");
    if (cap < f.hdr_bytes) return fail(NFEC_EINVAL, "nack_header_write_host: cap below the header's length");
    uint8_t* b = static_cast<uint8_t*>(out);
    put_word(b, ctl_header_word0(kNackVersionType, f.hdr_bytes, nack_sequence(f, i)));
    for (uint32_t j = 1; j < f.hdr_bytes / 4; ++j) put_word(b + 4 * j, f.w[j]);
    return (int)f.hdr_bytes;
}

extern "C" int nfec_nack_fragment_host(const void* content, uint64_t bytes, uint8_t fec_id, uint32_t segment_size,
                                       const nfec_nack_header* header, void* wire, uint64_t wire_bytes, uint32_t pitch,
                                       uint64_t* msg_offsets_out, uint16_t* msg_length_out, uint32_t capacity, uint64_t* totals)
{
    CtlHeaderFixed f;
    CutParams c;
    int rc = nack_header_fixed_from(header, f);
    if (rc || (rc = cut_params_from(fec_id, segment_size, f.hdr_bytes, c, "nack_fragment_host"))) return rc;
    if (!totals) return fail(NFEC_EINVAL, "nack_fragment_host: null totals");
    if (bytes && !content) return fail(NFEC_EINVAL, "nack_fragment_host: null content");
    if (bytes >> 32) return fail(NFEC_ERANGE, "nack_fragment_host: content of 2^32 bytes or more");
    if ((pitch & 3u) || pitch < f.hdr_bytes + c.S) return fail(NFEC_EINVAL, "nack_fragment_host: pitch is no multiple of 4 or below header + segment_size");
    if (capacity && !wire) return fail(NFEC_EINVAL, "nack_fragment_host: null wire");
    const uint64_t room = std::min<uint64_t>(capacity, wire_bytes / pitch);
    const HostContent load{static_cast<const uint8_t*>(content)};
    std::vector<uint32_t> req;
    CutIndex x;
    index_requests(load, bytes, c.L, req, &x.end);
    x.req = req.data(), x.R = (uint32_t)req.size();
    uint64_t messages = 0, written = 0, splits = 0;
    uint8_t* out = static_cast<uint8_t*>(wire);
    uint64_t pos = x.R ? 4u : kCutDone;
    uint32_t r = 0;
    while (pos != kCutDone) {
        r = cut_owner(x, pos);
        const CutMessage m = cut_message(c, x, r, pos, load);
        if (messages < room) {
            uint8_t* at = out + messages * pitch;
            put_word(at, ctl_header_word0(kNackVersionType, f.hdr_bytes, nack_sequence(f, messages)));
            for (uint32_t j = 1; j < f.hdr_bytes / 4; ++j) put_word(at + 4 * j, f.w[j]);
            put_content(m, load.bytes, at + f.hdr_bytes);
            if (msg_offsets_out) msg_offsets_out[messages] = messages * pitch;
            if (msg_length_out) msg_length_out[messages] = (uint16_t)(f.hdr_bytes + m.length);
        }
        ++messages, written += m.length, splits += m.split;
        pos = m.next;
    }
    totals[0] = messages, totals[1] = written, totals[2] = x.R, totals[3] = splits, totals[4] = x.end;
    totals[5] = x.end != bytes;
    return NFEC_OK;
}

extern "C" int nfec_adv_message_host(const void* content, uint64_t bytes, uint8_t fec_id, uint32_t segment_size,
                                     const nfec_adv_header* header, void* wire, uint64_t wire_bytes, uint64_t* totals)
{
    CtlHeaderFixed f;
    CutParams c;
    int rc = adv_header_fixed_from(header, f);
    if (rc || (rc = cut_params_from(fec_id, segment_size, f.hdr_bytes, c, "adv_message_host"))) return rc;
    if (!totals) return fail(NFEC_EINVAL, "adv_message_host: null totals");
    if (bytes && !content) return fail(NFEC_EINVAL, "adv_message_host: null content");
    if (bytes >> 32) return fail(NFEC_ERANGE, "adv_message_host: content of 2^32 bytes or more");
    if (!wire || wire_bytes < (uint64_t)f.hdr_bytes + c.S) return fail(NFEC_EINVAL, "adv_message_host: null wire, or wire_bytes below header + segment_size");
    const HostContent load{static_cast<const uint8_t*>(content)};
    totals[0] = 0, totals[1] = bytes, totals[2] = bytes != 0;
    const CutMessage m = cut_first_message(c, bytes, load);
    if (!m.length) return 0;
    const uint64_t used = m.used;
    const uint32_t limit = used != bytes;
    uint8_t* out = static_cast<uint8_t*>(wire);
    for (uint32_t j = 0; j < f.hdr_bytes / 4; ++j) put_word(out + 4 * j, j == 3 ? adv_flags_word(limit) : f.w[j]);
    put_content(m, load.bytes, out + f.hdr_bytes);
    totals[0] = m.length, totals[1] = bytes - used, totals[2] = limit;
    return (int)(f.hdr_bytes + m.length);
}

extern "C" int nfec_ctl_parse_host(const nfec_ctl_filter* filter, const void* wire, uint64_t wire_bytes, const uint64_t* offsets,
                                   const uint16_t* length, uint32_t count, uint8_t* class_out, uint64_t* content_offset_out,
                                   uint16_t* content_length_out, uint32_t* source_id_out, uint32_t* grtt_response_out,
                                   uint32_t* stats)
{
    CtlFilter f;
    const int rc = ctl_filter_from(filter, f);
    if (rc) return rc;
    if (count == 0) return 0;
    if (count > 0x7fffffffu) return fail(NFEC_ERANGE, "ctl_parse_host: count above 2^31 - 1");
    if (!wire || !offsets || !length) return fail(NFEC_EINVAL, "ctl_parse_host: null wire, offsets or length");
    const uint8_t* bytes = static_cast<const uint8_t*>(wire);
    int taken = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint64_t off = offsets[i];
        const uint32_t len = length[i];
        CtlParse p;
        p.cls = CTL_UNREADABLE, p.extended = 0, p.hdr_bytes = 0, p.source_id = 0, p.sec = p.usec = 0;
        const bool readable = ctl_readable(off, len, wire_bytes);
        if (readable) {
            uint32_t h[kCtlParseWords] = {0, 0, 0, 0, 0, 0};
            const uint32_t n = len < kCtlParseBytes ? len : kCtlParseBytes;
            for (uint32_t j = 0; j < n; ++j) h[j >> 2] |= (uint32_t)bytes[off + j] << (8u * (j & 3u));
            p = ctl_parse(h, len, f);
        }
        if (class_out) class_out[i] = (uint8_t)(p.cls | (p.extended ? CTL_EXTENDED : 0u));
        if (content_offset_out) content_offset_out[i] = p.hdr_bytes ? off + p.hdr_bytes : 0u;
        if (content_length_out) content_length_out[i] = (uint16_t)(p.hdr_bytes ? len - p.hdr_bytes : 0u);
        if (source_id_out) source_id_out[i] = p.source_id;
        if (grtt_response_out) grtt_response_out[2 * (size_t)i] = p.sec, grtt_response_out[2 * (size_t)i + 1] = p.usec;
        if (stats) ++stats[p.cls];
        taken += p.hdr_bytes != 0;
    }
    return taken;
}
