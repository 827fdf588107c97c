// ctl_msg_asan.cpp -- the host twins of the NORM_NACK / REPAIR_ADV message calls
// (norm_amd/csrc/ctl_msg_host.cpp over the headers, the cut and the parse of ctl_msg.hpp) under
// AddressSanitizer and UBSan.  Every content buffer lies in an allocation of exactly its length, so
// a cut that read a request header or a unit past the content's end -- behind a malformed tail, or
// where the last request ends on the last byte -- would be reported; every wire buffer holds exactly
// capacity * pitch bytes (the advertisement's exactly header + segment_size); every header is written
// into an allocation of exactly its length; and every datagram of the intake's table lies in an
// allocation of exactly its length, so a parse that read a sender_id, a flavor or a grtt_response
// that is not there would be reported.  Host code only, no GPU;
// `make -C tests/native -f ctl_msg_asan.mk`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ctl_msg.hpp"
#include "nfec.h"

// the library's error sink, which the entries under test report to
namespace nfec {
int fail(int code, const std::string& msg)
{
    (void)msg;
    return code;
}
}  // namespace nfec

using namespace nfec;

namespace {

int g_bad = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_bad;                                                  \
        }                                                             \
    } while (0)

uint32_t g_seed = 12345;
uint32_t rnd(uint32_t n)
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return (g_seed >> 8) % n;
}

// an allocation of exactly n bytes (one byte for n == 0, never read)
struct Exact {
    uint8_t* p;
    size_t n;
    explicit Exact(size_t bytes) : p(static_cast<uint8_t*>(std::malloc(bytes ? bytes : 1))), n(bytes) {}
    Exact(const std::vector<uint8_t>& v) : Exact(v.size())
    {
        if (n) std::memcpy(p, v.data(), n);
    }
    ~Exact() { std::free(p); }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
};

void put_request(std::vector<uint8_t>& out, uint32_t form, uint32_t flags, uint32_t units, uint32_t fec_id, uint32_t L)
{
    const uint32_t per = form == REPAIR_RANGES ? 2u : 1u, len = units * per * L;
    out.push_back((uint8_t)form), out.push_back((uint8_t)flags), out.push_back((uint8_t)(len >> 8)), out.push_back((uint8_t)len);
    for (uint32_t i = 0; i < units * per; ++i) {
        out.push_back((uint8_t)fec_id), out.push_back(0), out.push_back((uint8_t)rnd(256)), out.push_back((uint8_t)rnd(256));
        for (uint32_t j = 4; j < L; ++j) out.push_back((uint8_t)rnd(256));
    }
}

nfec_nack_header nack_header(bool ext)
{
    nfec_nack_header h;
    std::memset(&h, 0, sizeof h);
    h.source_id = 0x0A0B0C0Du, h.sender_id = 0x11223344u, h.instance_id = 0x5566, h.first_sequence = 65530, h.sequence_step = 3;
    h.grtt_response_sec = 7, h.grtt_response_usec = 9;
    if (ext) {
        for (int j = 0; j < 12; ++j) h.ext[j] = (uint8_t)(0xE0 + j);
        h.ext_bytes = 12;
    }
    return h;
}

// the units nack_parse reads of content (its fec_id is the content's)
uint64_t units_of(uint32_t fec_id, uint32_t fec_m, const uint8_t* content, uint64_t bytes)
{
    return nack_parse(fec_id, payload_id_kind((uint8_t)fec_id, (uint8_t)fec_m), content, bytes, nullptr, nullptr, nullptr, nullptr, 0, nullptr);
}

void fragment_case(const std::vector<uint8_t>& content, uint64_t good_bytes, uint32_t fec_id, uint32_t fec_m, uint32_t S, bool ext)
{
    const nfec_nack_header h = nack_header(ext);
    const uint32_t H = (uint32_t)nfec_nack_header_bytes(h.ext_bytes), pitch = H + S;
    const Exact c(content);
    const uint32_t cap = (uint32_t)(content.size() / 8 + 2);
    Exact wire((size_t)cap * pitch);
    std::vector<uint64_t> off(cap);
    std::vector<uint16_t> len(cap);
    uint64_t totals[6];
    CHECK(nfec_nack_fragment_host(c.p, c.n, (uint8_t)fec_id, S, &h, wire.p, wire.n, pitch, off.data(), len.data(), cap, totals) == NFEC_OK);
    CHECK(totals[0] <= cap && totals[4] == good_bytes && totals[5] == (good_bytes != content.size()));
    std::vector<uint8_t> joined;
    uint64_t written = 0;
    for (uint64_t i = 0; i < totals[0]; ++i) {
        CHECK(off[i] == i * pitch && len[i] > H && len[i] <= H + S);
        Exact head(H);
        CHECK(nfec_nack_header_write_host(&h, (uint32_t)i, head.p, head.n) == (int)H);
        CHECK(std::memcmp(head.p, wire.p + off[i], H) == 0);
        joined.insert(joined.end(), wire.p + off[i] + H, wire.p + off[i] + len[i]);
        written += len[i] - H;
    }
    CHECK(written == totals[1]);
    // the messages name the units of the content in front of the stop
    const Exact j(joined);
    CHECK(units_of(fec_id, fec_m, j.p, j.n) == units_of(fec_id, fec_m, c.p, good_bytes));
    // a capacity of one message, in a wire buffer of exactly one message
    Exact one(pitch);
    uint64_t t1[6];
    CHECK(nfec_nack_fragment_host(c.p, c.n, (uint8_t)fec_id, S, &h, one.p, one.n, pitch, off.data(), len.data(), 1, t1) == NFEC_OK);
    CHECK(std::memcmp(t1, totals, sizeof totals) == 0);
    if (totals[0]) CHECK(std::memcmp(one.p, wire.p, len[0]) == 0);

    // the advertisement: the header and the first message of the same cut
    nfec_adv_header ah;
    std::memset(&ah, 0, sizeof ah);
    ah.source_id = 0x11223344u, ah.instance_id = 0x5566, ah.sequence = 9, ah.grtt = 0x40, ah.backoff = 4, ah.gsize = 1;
    if (ext) std::memcpy(ah.ext, h.ext, 12), ah.ext_bytes = 12;
    const uint32_t AH = (uint32_t)nfec_adv_header_bytes(ah.ext_bytes);
    Exact adv((size_t)AH + S);
    uint64_t at[3];
    const int n = nfec_adv_message_host(c.p, c.n, (uint8_t)fec_id, S, &ah, adv.p, adv.n, at);
    if (totals[0]) {
        CHECK(n == (int)(AH + len[0] - H) && std::memcmp(adv.p + AH, wire.p + H, len[0] - H) == 0);
        CHECK(adv.p[13] == (at[1] ? 1 : 0) && at[2] == (at[1] ? 1u : 0u) && at[0] == (uint64_t)len[0] - H);
    } else {
        CHECK(n == 0 && at[0] == 0 && at[1] == content.size());
    }
}

void fragment_cases()
{
    const struct {
        uint32_t fec_id, fec_m, L;
    } forms[] = {{5, 8, 8}, {2, 16, 8}, {129, 8, 12}};
    const uint32_t sizes[] = {40, 44, 64, 104, 1400};
    for (const auto& f : forms)
        for (uint32_t S : sizes) {
            if (S < 4 + 2 * f.L) continue;
            for (int t = 0; t < 40; ++t) {
                std::vector<uint8_t> content;
                const uint32_t n = 1 + rnd(12);
                for (uint32_t r = 0; r < n; ++r)
                    put_request(content, 1 + rnd(2), rnd(8), rnd(10) ? rnd(S <= 104 ? 6 : 60) : 0, f.fec_id, f.L);
                const uint64_t good = content.size();
                fragment_case(content, good, f.fec_id, f.fec_m, S, t & 1);
                // the malformed tails: a length past the content, item bytes that are no multiple of L, an odd
                // item count in RANGES, a header that does not fit
                std::vector<uint8_t> bad = content;
                switch (t & 3) {
                case 0: bad.insert(bad.end(), {1, 1, 0, (uint8_t)(2 * f.L)}), bad.resize(bad.size() + f.L); break;
                case 1: bad.insert(bad.end(), {1, 1, 0, (uint8_t)(f.L + 4)}), bad.resize(bad.size() + f.L + 4); break;
                case 2: bad.insert(bad.end(), {2, 1, 0, (uint8_t)(3 * f.L)}), bad.resize(bad.size() + 3 * f.L); break;
                default: bad.insert(bad.end(), {1, 1, 0}); break;
                }
                fragment_case(bad, good, f.fec_id, f.fec_m, S, t & 2);
            }
        }
    // what the calls refuse
    const nfec_nack_header h = nack_header(false);
    uint64_t totals[6];
    uint8_t byte[4] = {0, 0, 0, 0};
    CHECK(nfec_nack_fragment_host(byte, 0, 5, 42, &h, byte, 0, 68, nullptr, nullptr, 0, totals) == NFEC_EINVAL);
    CHECK(nfec_nack_fragment_host(byte, 0, 5, 16, &h, byte, 0, 40, nullptr, nullptr, 0, totals) == NFEC_EINVAL);
    CHECK(nfec_nack_fragment_host(byte, 0, 5, 65512, &h, byte, 0, 65536, nullptr, nullptr, 0, totals) == NFEC_EINVAL);
    CHECK(nfec_nack_fragment_host(byte, 0, 5, 40, &h, byte, 0, 60, nullptr, nullptr, 0, totals) == NFEC_EINVAL);
    CHECK(nfec_nack_fragment_host(byte, 0, 7, 40, &h, byte, 0, 64, nullptr, nullptr, 0, totals) == NFEC_EINVAL);
    CHECK(nfec_nack_fragment_host(byte, 0, 5, 40, &h, byte, 0, 64, nullptr, nullptr, 0, totals) == NFEC_OK && totals[0] == 0);
    CHECK(nfec_nack_header_bytes(8) == NFEC_EINVAL && nfec_adv_header_bytes(16) == NFEC_EINVAL);
    CHECK(nfec_nack_header_bytes(12) == 36 && nfec_adv_header_bytes(12) == 28);
    Exact small(23);
    CHECK(nfec_nack_header_write_host(&h, 0, small.p, small.n) == NFEC_EINVAL);
}

// ---- the intake ----

std::vector<uint8_t> nack_dgram(uint32_t hdr_len, uint32_t source, uint32_t sender, uint32_t instance, size_t total)
{
    std::vector<uint8_t> d = {0x14, (uint8_t)hdr_len, 0, 5};
    for (uint32_t v : {source, sender}) d.insert(d.end(), {(uint8_t)(v >> 24), (uint8_t)(v >> 16), (uint8_t)(v >> 8), (uint8_t)v});
    d.insert(d.end(), {(uint8_t)(instance >> 8), (uint8_t)instance, 0, 0, 0, 0, 0, 7, 0, 0, 0, 9});
    while (d.size() < total) d.push_back((uint8_t)(0xE0 + d.size()));
    d.resize(total);
    return d;
}

std::vector<uint8_t> adv_dgram(uint32_t hdr_len, uint32_t source, uint32_t instance, uint32_t flavor, size_t total)
{
    std::vector<uint8_t> d = {0x13, (uint8_t)hdr_len, 0, 5};
    d.insert(d.end(), {(uint8_t)(source >> 24), (uint8_t)(source >> 16), (uint8_t)(source >> 8), (uint8_t)source});
    d.insert(d.end(), {(uint8_t)(instance >> 8), (uint8_t)instance, 1, 2, (uint8_t)flavor, 0, 0, 0});
    while (d.size() < total) d.push_back((uint8_t)(0xE0 + d.size()));
    d.resize(total);
    return d;
}

void parse_one(const std::vector<uint8_t>& d, uint32_t flags, uint32_t want_cls, uint32_t want_hdr)
{
    const Exact wire(d);
    nfec_ctl_filter f;
    std::memset(&f, 0, sizeof f);
    f.sender_id = 0x11223344u, f.instance_id = 0x5566, f.local_id = 0x0A0B0C0Du, f.flags = flags;
    const uint64_t off = 0;
    const uint16_t len = (uint16_t)d.size();
    uint8_t cls = 0xff;
    uint64_t coff = ~(uint64_t)0;
    uint16_t clen = 0xffff;
    uint32_t src = 0, grtt[2] = {1, 1}, stats[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int taken = nfec_ctl_parse_host(&f, wire.p, wire.n, &off, &len, 1, &cls, &coff, &clen, &src, grtt, stats);
    CHECK(cls == want_cls);
    CHECK(taken == (want_hdr ? 1 : 0) && coff == want_hdr && clen == (want_hdr ? d.size() - want_hdr : 0));
    CHECK(stats[cls & 0x7f] == 1);
}

void intake_cases()
{
    const uint32_t sender = 0x11223344u, inst = 0x5566, other = 0x01010101u, local = 0x0A0B0C0Du;
    const uint32_t take_n = NFEC_CTL_TAKE_NACK, take_a = NFEC_CTL_TAKE_ADV;
    // every length 0 .. 40, with and without the extension, each datagram alone in its allocation
    for (size_t n = 0; n <= 40; ++n) {
        parse_one(nack_dgram(6, other, sender, inst, n), take_n, n < 8 ? NFEC_CTL_UNREADABLE : n < 24 ? NFEC_CTL_MALFORMED : NFEC_CTL_NACK,
                  n < 24 ? 0 : 24);
        parse_one(nack_dgram(9, other, sender, inst, n), take_n,
                  n < 8 ? NFEC_CTL_UNREADABLE : n < 36 ? NFEC_CTL_MALFORMED : NFEC_CTL_NACK | NFEC_CTL_EXTENDED, n < 36 ? 0 : 36);
        parse_one(adv_dgram(4, sender, inst, 5, n), take_a, n < 8 ? NFEC_CTL_UNREADABLE : n < 16 ? NFEC_CTL_MALFORMED : NFEC_CTL_REPAIR_ADV,
                  n < 16 ? 0 : 16);
        parse_one(adv_dgram(7, sender, inst, 5, n), take_a,
                  n < 8 ? NFEC_CTL_UNREADABLE : n < 28 ? NFEC_CTL_MALFORMED : NFEC_CTL_REPAIR_ADV | NFEC_CTL_EXTENDED, n < 28 ? 0 : 28);
        // a sender takes NACKs only, a receiver advertisements only
        parse_one(nack_dgram(6, other, sender, inst, n), take_a, n < 8 ? NFEC_CTL_UNREADABLE : n < 24 ? NFEC_CTL_MALFORMED : NFEC_CTL_NACK, 0);
    }
    parse_one(nack_dgram(5, other, sender, inst, 28), take_n, NFEC_CTL_MALFORMED, 0);   // hdr_len too small
    parse_one(adv_dgram(3, sender, inst, 5, 20), take_a, NFEC_CTL_MALFORMED, 0);
    parse_one(nack_dgram(8, other, sender, inst, 28), take_n, NFEC_CTL_MALFORMED, 0);   // ... too large
    parse_one(adv_dgram(6, sender, inst, 5, 20), take_a, NFEC_CTL_MALFORMED, 0);
    std::vector<uint8_t> data = nack_dgram(6, other, sender, inst, 28);
    data[0] = 0x12;
    parse_one(data, take_n, NFEC_CTL_OTHER_TYPE, 0);
    parse_one(adv_dgram(4, sender, inst, 4, 20), take_a, NFEC_CTL_OTHER_FLAVOR, 0);
    parse_one(nack_dgram(6, local, sender, inst, 28), take_n, NFEC_CTL_OWN, 0);
    parse_one(adv_dgram(4, local, inst, 5, 20), take_a, NFEC_CTL_OWN, 0);
    parse_one(nack_dgram(6, other, sender + 1, inst, 28), take_n, NFEC_CTL_OTHER_SENDER, 0);
    parse_one(adv_dgram(4, sender + 1, inst, 5, 20), take_a, NFEC_CTL_OTHER_SENDER, 0);
    parse_one(nack_dgram(6, other, sender, inst + 1, 28), take_n, NFEC_CTL_OTHER_INSTANCE, 0);
    parse_one(adv_dgram(4, sender, inst + 1, 5, 20), take_a, NFEC_CTL_OTHER_INSTANCE, 0);
    parse_one(nack_dgram(6, other, sender, inst + 1, 28), take_n | NFEC_CTL_ANY_INSTANCE, NFEC_CTL_NACK, 24);
    parse_one(adv_dgram(4, sender, inst + 1, 5, 20), take_a | NFEC_CTL_ANY_INSTANCE, NFEC_CTL_REPAIR_ADV, 16);
}

}  // namespace

int main()
{
    fragment_cases();
    intake_cases();
    if (g_bad) {
        std::printf("%d checks failed\n", g_bad);
        return 1;
    }
    std::printf("control message driver done\n");
    return 0;
}
