// nack_walk_asan.cpp -- the per-block walk of the repair requests and the parser of their content
// (norm_amd/csrc/nack_layout.hpp, what nfec_rx_repair_requests_host and nfec_repair_parse_host run)
// as host code under AddressSanitizer and UBSan, with every byte a call may not touch poisoned.
// The block's mask words, the content buffer and the parser's item array each end their
// allocation (a block's numData reaches the walk by value); the mask words behind (nd + m + 31) / 32, the content at or past its capacity and
// the bytes behind what a parser was given are closed.  What is checked: a walk reads only the
// block's words and writes only below the capacity, whatever the total; its content parses back to
// exactly the slots the rule asks for; and content that claims too much (a length field past the
// end, a header cut short, units past the arrays' capacity) makes the parser touch nothing outside.
// Host code only, no GPU; `make -C tests/native -f nack_walk_asan.mk`.
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "nack_layout.hpp"

using namespace nfec;

namespace {

// A page-aligned buffer whose last byte is the allocation's last: a case uses the last bytes of it.
struct Arena {
    uint8_t* p;
    size_t n;
    explicit Arena(size_t bytes) : n((bytes + 4095) & ~(size_t)4095)
    {
        p = static_cast<uint8_t*>(aligned_alloc(4096, n));
        if (!p) abort();
        std::memset(p, 0xEE, n);
    }
    ~Arena()
    {
        __asan_unpoison_memory_region(p, n);
        free(p);
    }
    uint8_t* tail(size_t bytes) const { return p + n - bytes; }
    // only [at, at + bytes) stays open
    void only(const void* at, size_t bytes)
    {
        __asan_poison_memory_region(p, n);
        __asan_unpoison_memory_region(at, bytes);
    }
    void open_all() { __asan_unpoison_memory_region(p, n); }
};

int failures = 0;
void fail(const char* what, uint32_t a, uint32_t b)
{
    if (failures++ < 20) std::printf("%s: %u %u\n", what, a, b);
}

uint32_t rnd(uint64_t& s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
}

NackFormat format(uint8_t fec_id, uint8_t fec_m, uint32_t max_units)
{
    NackFormat f;
    f.id_kind = payload_id_kind(fec_id, fec_m);
    f.item_len = nack_item_length(f.id_kind);
    f.fec_id = fec_id, f.object_id = 0x0102, f.first_block_id = 0, f.max_units = max_units;
    return f;
}

// the slots the rule asks for, by the sentences of nfec.h
std::set<uint32_t> asked_for(const std::vector<bool>& got, uint32_t nd, uint32_t m)
{
    std::vector<uint32_t> pend;
    uint32_t e = 0;
    for (uint32_t s = 0; s < nd + m; ++s)
        if (!got[s]) pend.push_back(s), e += s < nd;
    std::set<uint32_t> out;
    if (e > m) {
        out.insert(pend.begin() + m, pend.end());
    } else {
        for (uint32_t s : pend)
            if (s >= nd && s < nd + e) out.insert(s);
    }
    return out;
}

void walk_cases()
{
    uint64_t seed = 7;
    struct Shape {
        uint32_t k, m;
        uint8_t fec_id, fec_m;
    };
    for (Shape sh : {Shape{4, 2, 5, 8}, Shape{8, 4, 2, 8}, Shape{64, 32, 129, 8}, Shape{200, 55, 5, 8}, Shape{4096, 256, 2, 16}})
        for (uint32_t trial = 0; trial < (sh.k > 1000 ? 12u : 60u); ++trial) {
            const uint32_t nd = trial % 3 ? sh.k : sh.k - 1, n = nd + sh.m, nwords = (n + 31) / 32;
            const uint32_t loss = 5 + rnd(seed) % 91;
            std::vector<bool> got(n);
            for (uint32_t s = 0; s < n; ++s) got[s] = rnd(seed) % 100 >= loss;
            // the mask: exactly the block's words, ending the allocation; bits at or past n are noise
            Arena marena((size_t)nwords * 4), carena(1 << 18);
            uint32_t* mask = reinterpret_cast<uint32_t*>(marena.tail((size_t)nwords * 4));
            for (uint32_t w = 0; w < nwords; ++w) mask[w] = rnd(seed);
            for (uint32_t s = 0; s < n; ++s)
                mask[s >> 5] = (mask[s >> 5] & ~(1u << (s & 31u))) | ((uint32_t)got[s] << (s & 31u));
            marena.only(mask, (size_t)nwords * 4);
            NackCut cut = {0, 0};
            const uint32_t cls = nack_block_class_host(mask, nd, sh.k, sh.m, &cut);
            const std::set<uint32_t> want = asked_for(got, nd, sh.m);
            if (cls == NACK_NEEDING && want.empty()) fail("class", sh.k, trial);  // (pigeonhole on p < e)
            if (cls != NACK_NEEDING) continue;
            const NackFormat f = format(sh.fec_id, sh.fec_m, 1 + trial % 5);
            // the total first (capacity 0 writes nothing), then capacities below and at it
            NackWriter count;
            nack_block_emit_host(mask, nd, cut, 3, f, count);
            const uint64_t total = count.off;
            for (uint64_t cap : {(uint64_t)0, (uint64_t)5, total / 2, total - 1, total}) {
                if (cap > total) continue;
                NackWriter o;
                o.content = carena.tail(cap), o.capacity = cap;
                carena.open_all();
                std::memset(carena.p, 0xEE, carena.n);
                carena.only(o.content, cap);
                nack_block_emit_host(mask, nd, cut, 3, f, o);
                if (o.off != total || o.requests != count.requests) fail("total", sh.k, trial);
                if (cap != total) continue;
                // the content parses back to the request set
                std::vector<NackItem> first(total / 8 + 1), last(total / 8 + 1);
                std::vector<uint8_t> flags(first.size()), form(first.size());
                uint64_t consumed = 0;
                const uint64_t units = nack_parse(sh.fec_id, f.id_kind, o.content, total, flags.data(), form.data(), first.data(),
                                                  last.data(), first.size(), &consumed);
                if (consumed != total) fail("consumed", sh.k, trial);
                std::set<uint32_t> have;
                for (uint64_t u = 0; u < units; ++u) {
                    if (flags[u] != REPAIR_SEGMENT || first[u].block_id != 3 || last[u].block_id != 3) fail("unit", sh.k, trial);
                    for (uint32_t s = first[u].symbol; s <= last[u].symbol; ++s) have.insert(s);
                }
                if (have != want) fail("request set", sh.k, trial);
            }
            marena.open_all(), carena.open_all();
        }
}

void parse_cases()
{
    // four requests of one block, fec_id 129 (12-byte items)
    const uint32_t k = 64, m = 4, nd = 64, nwords = 3;
    std::vector<uint32_t> mask(nwords, 0xffffffffu);
    for (uint32_t s : {0u, 1u, 2u, 3u, 10u, 12u, 13u, 20u, 21u, 22u, 23u, 24u, 30u}) mask[s >> 5] &= ~(1u << (s & 31u));
    NackCut cut = {0, 0};
    if (nack_block_class_host(mask.data(), nd, k, m, &cut) != NACK_NEEDING) fail("parse setup", 0, 0);
    const NackFormat f = format(129, 8, 100);
    std::vector<uint8_t> good(256);
    NackWriter o;
    o.content = good.data(), o.capacity = good.size();
    nack_block_emit_host(mask.data(), nd, cut, 0, f, o);
    const uint64_t total = o.off;  // ITEMS x3 items, RANGES, ITEMS
    if (total != 4 + 36 + 4 + 24 + 4 + 12) fail("parse setup total", (uint32_t)total, 0);

    Arena carena(4096), oarena(1 << 16);
    auto run = [&](const std::vector<uint8_t>& bytes, uint64_t len, uint32_t capacity, uint64_t want_units, uint64_t want_consumed) {
        uint8_t* c = carena.tail(len);
        carena.open_all();
        std::memcpy(c, bytes.data(), len);
        carena.only(c, len);
        // the item array ends its allocation; the flags have one element to spare
        NackItem* first = reinterpret_cast<NackItem*>(oarena.tail((size_t)capacity * sizeof(NackItem)));
        oarena.only(first, (size_t)capacity * sizeof(NackItem));
        std::vector<uint8_t> flags(capacity + 1);
        uint64_t consumed = ~0ull;
        const uint64_t units = nack_parse(129, f.id_kind, c, len, flags.data(), nullptr, first, nullptr, capacity, &consumed);
        if (units != want_units || consumed != want_consumed) fail("parse", (uint32_t)units, (uint32_t)consumed);
        carena.open_all(), oarena.open_all();
    };
    run(good, total, 16, 5, total);
    run(good, total, 2, 5, total);    // units past the arrays' capacity are counted, not written
    run(good, total, 0, 5, total);
    for (uint64_t len = 0; len < total; ++len) {  // every truncation stops at a request's header
        const uint64_t at = len < 40 ? 0 : len < 68 ? 40 : len < 84 ? 68 : 84;
        const uint64_t units = len < 40 ? 0 : len < 68 ? 3 : len < 84 ? 4 : 5;
        run(good, len, 16, units, at == 84 ? 84 : at);
    }
    std::vector<uint8_t> bad = good;
    bad[2] = 0xff, bad[3] = 0xff;  // a length field that claims 65,535 bytes
    run(bad, total, 16, 0, 0);
    bad = good;
    bad[42] = 0, bad[43] = 28;     // the RANGES request claims four bytes more than the content holds
    run(bad, 40 + 4 + 24, 16, 3, 40);
    bad = good;
    bad[40 + 4 + 12] = 5;          // a foreign fec_id in the range's second item
    run(bad, total, 16, 3, 44);
    bad = good;
    bad[42] = 0, bad[43] = 12;     // a RANGES request with one item
    run(bad, total, 16, 3, 40);
}

}  // namespace

int main()
{
    walk_cases();
    parse_cases();
    if (failures) {
        std::printf("%d cases failed\n", failures);
        return 1;
    }
    std::printf("nack walk driver done\n");
    return 0;
}
