// data_msg_asan.cpp -- the host twins of the NORM_DATA message calls (norm_amd/csrc/data_msg_host.cpp
// over the header and the parse of data_msg.hpp) and the scatter rule's header form
// (segment_copy.hpp: scatter_header_image, scatter_piece_header) under AddressSanitizer and UBSan.
// Every datagram of the malformed table lies in an allocation of exactly its length, so a parse that
// read a byte past a datagram's end -- a fec_id byte, an ID or an extension word that is not there --
// would be reported; every header is written into an allocation of exactly its length; and every
// message of the scatter cases reads a slot of exactly its length rounded up to 8, with the bytes in
// front of and behind the message checked against a fill.  Host code only, no GPU; `make -C tests/native -f data_msg_asan.mk`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "data_msg.hpp"
#include "nfec.h"
#include "segment_copy.hpp"

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

constexpr uint32_t kSource = 0xC0A80107u;
constexpr uint16_t kInstance = 0xBEEF, kObject = 0x8123;

struct Form {
    uint8_t fec_id, fec_m;
    uint32_t idlen;
};
const Form kForms[] = {{5, 8, 4}, {2, 8, 4}, {2, 16, 4}, {129, 8, 8}};

nfec_data_header header_for(const Form& f, bool with_fti)
{
    nfec_data_header h;
    std::memset(&h, 0, sizeof h);
    h.source_id = kSource, h.instance_id = kInstance, h.object_id = kObject;
    h.first_sequence = 65534, h.grtt = 0x9C, h.backoff = 5, h.gsize = 3, h.flags = 0x1A;
    h.fec_id = f.fec_id, h.fec_m = f.fec_m;
    if (with_fti) {
        nfec_fti fti;
        std::memset(&fti, 0, sizeof fti);
        fti.fec_id = f.fec_id, fti.fec_m = f.fec_m, fti.fec_group_size = 1;
        fti.segment_size = 1392, fti.num_data = 64, fti.num_parity = 32, fti.object_size = 0x123456789AULL;
        const int n = nfec_fti_write(&fti, h.ext, sizeof h.ext);
        if (n <= 0) abort();
        h.ext_bytes = (uint8_t)n;
    }
    return h;
}

// one datagram in an allocation of exactly its length, parsed alone
struct Parsed {
    uint8_t cls;
    uint16_t seq, sym, blen, plen;
    uint32_t blk;
    uint64_t poff, fti;
};
Parsed parse_exact(const Form& f, const std::vector<uint8_t>& bytes)
{
    uint8_t* exact = static_cast<uint8_t*>(std::malloc(bytes.size() ? bytes.size() : 1));
    if (!exact) abort();
    if (!bytes.empty()) std::memcpy(exact, bytes.data(), bytes.size());
    nfec_data_filter flt = {kSource, kInstance, f.fec_id, f.fec_m, kObject};
    const uint64_t off = 0;
    const uint16_t len = (uint16_t)bytes.size();
    Parsed p;
    std::memset(&p, 0xCC, sizeof p);
    const int rc = nfec_rx_parse_data_host(&flt, 0, exact, bytes.size(), &off, &len, 1, &p.cls, &p.seq, &p.blk, &p.sym,
                                           &p.blen, &p.poff, &p.plen, &p.fti);
    CHECK(rc == (p.cls == NFEC_DGRAM_PARSED ? 1 : 0));
    std::free(exact);
    return p;
}

std::vector<uint8_t> datagram(const Form& f, bool with_fti, int hdr_len, size_t payload)
{
    const nfec_data_header h = header_for(f, with_fti);
    std::vector<uint8_t> d(40);
    const int n = nfec_data_header_write_host(&h, 1, 7, 3, 8, d.data(), d.size());
    if (n <= 0) abort();
    d.resize((size_t)n);
    if (hdr_len >= 0) d[1] = (uint8_t)hdr_len;
    for (size_t j = 0; j < payload; ++j) d.push_back((uint8_t)(j + 1));
    return d;
}

void parse_cases()
{
    for (const Form& f : kForms) {
        const uint32_t base = 16 + f.idlen, words = base / 4;
        // InitFromBuffer's bounds from both sides
        CHECK(parse_exact(f, datagram(f, false, (int)words - 1, 8)).cls == NFEC_DGRAM_MALFORMED);
        Parsed p = parse_exact(f, datagram(f, false, (int)words, 8));
        CHECK(p.cls == NFEC_DGRAM_PARSED && p.poff == base && p.plen == 8 && p.blk == 7 && p.sym == 3 && p.fti == ~0ull);
        CHECK(p.seq == 65535);
        CHECK(parse_exact(f, datagram(f, false, (int)words + 3, 8)).cls == NFEC_DGRAM_MALFORMED);
        p = parse_exact(f, datagram(f, false, (int)words + 2, 8));
        CHECK(p.cls == NFEC_DGRAM_PARSED && p.poff == base + 8 && p.plen == 0);
        p = parse_exact(f, datagram(f, false, -1, 0));  // exactly 16 + idlen bytes
        CHECK(p.cls == NFEC_DGRAM_PARSED && p.poff == base && p.plen == 0);
        CHECK(p.blen == (f.fec_id == 129 ? 8 : 0));
        // every length below the base header, with a header that claims everything is there
        for (uint32_t cut = 0; cut < base; ++cut) {
            std::vector<uint8_t> d = datagram(f, true, -1, 0);
            d.resize(cut);
            p = parse_exact(f, d);
            CHECK(p.cls == (cut < 8 ? NFEC_DGRAM_UNREADABLE : NFEC_DGRAM_MALFORMED));
            CHECK(p.blk == 0xffffffffu && p.sym == 0xffff && p.poff == 0 && p.plen == 0);
        }
        // ... and every length from there to the whole header: the header runs past the datagram
        const uint32_t full = base + header_for(f, true).ext_bytes;
        for (uint32_t cut = base; cut <= full + 2; ++cut) {
            std::vector<uint8_t> d = datagram(f, true, -1, 2);
            d.resize(cut);
            p = parse_exact(f, d);
            CHECK(p.cls == (cut < full ? NFEC_DGRAM_MALFORMED : NFEC_DGRAM_PARSED));
            if (cut >= full) CHECK(p.fti == 0 && p.poff == full && p.plen == cut - full);
        }
        // fec_id bytes 0 and 3
        for (uint8_t id : {(uint8_t)0, (uint8_t)3}) {
            std::vector<uint8_t> d = datagram(f, false, -1, 12);
            d[13] = id;
            CHECK(parse_exact(f, d).cls == NFEC_DGRAM_MALFORMED);
        }
        // the first extension: a length byte of 0, one that runs past the header, an unknown type
        std::vector<uint8_t> d = datagram(f, true, -1, 4);
        d[base + 1] = 0;
        p = parse_exact(f, d);
        CHECK(p.cls == NFEC_DGRAM_PARSED && p.fti == ~0ull);
        d = datagram(f, true, -1, 4);
        d[base + 1] = (uint8_t)(d[base + 1] + 1);
        CHECK(parse_exact(f, d).fti == ~0ull);
        d = datagram(f, true, -1, 4);
        d[base] = 1;
        CHECK(parse_exact(f, d).fti == ~0ull);
        // the other classes, on exact allocations too
        d = datagram(f, false, -1, 4);
        d[0] = 0x14;
        CHECK(parse_exact(f, d).cls == NFEC_DGRAM_OTHER_TYPE);
        d.resize(8);
        CHECK(parse_exact(f, d).cls == NFEC_DGRAM_OTHER_TYPE);
        d = datagram(f, false, -1, 4);
        d[7] ^= 1;
        CHECK(parse_exact(f, d).cls == NFEC_DGRAM_OTHER_SENDER);
        d = datagram(f, false, -1, 4);
        d[15] ^= 1;
        CHECK(parse_exact(f, d).cls == NFEC_DGRAM_OTHER_OBJECT);
        d = datagram(f, false, -1, 8);
        d[13] = f.fec_id == 129 ? 5 : 129;
        if (f.fec_id != 129) d[1] = 6;  // (a header that holds the longer ID: another code's, not a malformed one)
        CHECK(parse_exact(f, d).cls == NFEC_DGRAM_OTHER_CODE);
    }
}

void header_cases()
{
    for (const Form& f : kForms)
        for (int with_fti = 0; with_fti < 2; ++with_fti) {
            const nfec_data_header h = header_for(f, with_fti != 0);
            const int want = nfec_data_header_bytes(f.fec_id, h.ext_bytes);
            CHECK(want == (int)(16 + f.idlen + h.ext_bytes));
            uint8_t* exact = static_cast<uint8_t*>(std::malloc((size_t)want));
            if (!exact) abort();
            CHECK(nfec_data_header_write_host(&h, 3, 0xABCDEF, 9, 8, exact, (size_t)want) == want);
            CHECK(exact[0] == 0x12 && exact[1] == want / 4 && exact[2] == 0 && exact[3] == 1);  // 65534 + 3
            CHECK(exact[13] == f.fec_id && !std::memcmp(exact + 16 + f.idlen, h.ext, h.ext_bytes));
            CHECK(nfec_data_header_write_host(&h, 3, 0xABCDEF, 9, 8, exact, (size_t)want - 1) == NFEC_EINVAL);
            std::free(exact);
        }
}

// the scatter rule's header form: every residue, every header length, payload lengths round the
// piece and chunk edges
void scatter_cases()
{
    const uint32_t lens[] = {0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40, 41, 100};
    for (const Form& f : kForms)
        for (int with_fti = 0; with_fti < 2; ++with_fti) {
            const nfec_data_header h = header_for(f, with_fti != 0);
            uint8_t hb[40];
            const uint32_t H = (uint32_t)nfec_data_header_write_host(&h, 5, 0x123456, 17, 8, hb, sizeof hb);
            uint32_t hw[kScatterHeaderWords] = {0};
            for (uint32_t j = 0; j < H; ++j) hw[j >> 2] |= (uint32_t)hb[j] << (8u * (j & 3u));
            for (uint32_t res = 0; res < 16; ++res)
                for (uint32_t len : lens) {
                    // the slot: its length rounded up to 8 and not a byte more (malloc aligns it to 16)
                    const size_t slot_bytes = len ? (len + 7u) & ~7u : 8u;
                    uint8_t* slot = static_cast<uint8_t*>(std::malloc(slot_bytes));
                    const size_t total = res + H + len, room = (total + 15u) & ~(size_t)15u;
                    uint8_t* buf = static_cast<uint8_t*>(aligned_alloc(16, room));
                    if (!slot || !buf) abort();
                    for (size_t j = 0; j < slot_bytes; ++j) slot[j] = (uint8_t)(0x40 + j * 7);
                    std::memset(buf, 0xA5, room);
                    uint8_t* dst = buf + res;
                    uint32_t img[16];
                    scatter_header_image(hw, res, img);
                    const uint32_t pieces = scatter_pieces(dst, H + len);
                    for (uint32_t p = 0; p < pieces + 2; ++p) scatter_piece_header(dst, slot, len, img, H, p);
                    bool same = !std::memcmp(dst, hb, H) && !std::memcmp(dst + H, slot, len);
                    for (uint32_t j = 0; j < res; ++j) same = same && buf[j] == 0xA5;
                    for (size_t j = total; j < room; ++j) same = same && buf[j] == 0xA5;
                    if (!same) {
                        std::printf("scatter mismatch: fec %u H %u res %u len %u\n", f.fec_id, H, res, len);
                        ++g_bad;
                    }
                    std::free(slot), std::free(buf);
                }
        }
}

}  // namespace

int main()
{
    parse_cases();
    header_cases();
    scatter_cases();
    if (g_bad) {
        std::printf("data message driver: %d checks failed\n", g_bad);
        return 1;
    }
    std::printf("data message driver done\n");
    return 0;
}
