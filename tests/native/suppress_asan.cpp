// suppress_asan.cpp -- NACK suppression and repair advertisements on the host (norm_amd/csrc/
// suppress_host.cpp and nack_host.cpp over the rule of suppress_layout.hpp:
// nfec_rx_handle_repair_content_host, nfec_rx_repair_pending_host and nfec_tx_repair_adv_host) under
// AddressSanitizer and UBSan, with every byte a call may not touch poisoned: the wire buffer is
// closed except for the messages themselves (each ends on an 8-byte boundary, so the byte behind it
// is closed exactly), and the reception mask, the three arrays of the receiver's state, the
// sender's state, numData, pending_blocks, the content, block_start and the totals each end their
// allocation.  What is checked besides the sanitizers' silence: self-suppression (a receiver that
// hears its own NACK stays silent), that the advertisement of a sender that handled that NACK
// suppresses it too where it names explicit segments, that handling in two orders gives one state,
// that damaged and unreadable messages are counted, that no bit at or past nd + m is set, and that
// the decision reads the state without changing it.  Host code only, no GPU;
// `make -C tests/native -f suppress_asan.mk`.
#include <sanitizer/asan_interface.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nfec.h"
#include "suppress_layout.hpp"

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

// A page-aligned buffer whose last byte is the allocation's last: a case uses the last bytes of it.
struct Arena {
    uint8_t* p;
    size_t n;
    explicit Arena(size_t bytes) : n((bytes + 4095) & ~(size_t)4095)
    {
        if (n == 0) n = 4096;
        p = static_cast<uint8_t*>(aligned_alloc(4096, n));
        if (!p) abort();
        std::memset(p, 0xEE, n);
    }
    ~Arena()
    {
        __asan_unpoison_memory_region(p, n);
        free(p);
    }
    template <typename T>
    T* tail(size_t count)
    {
        T* at = reinterpret_cast<T*>(p + n - count * sizeof(T));
        __asan_poison_memory_region(p, n);
        __asan_unpoison_memory_region(at, count * sizeof(T));
        return at;
    }
    void close() { __asan_poison_memory_region(p, n); }
    void open(const void* at, size_t bytes) { __asan_unpoison_memory_region(at, bytes); }
    void open_all() { __asan_unpoison_memory_region(p, n); }
};

int failures = 0;
void fail_case(const char* what, uint64_t a, uint64_t b)
{
    if (failures++ < 20) std::printf("%s: %llu %llu\n", what, (unsigned long long)a, (unsigned long long)b);
}

uint32_t rnd(uint64_t& s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
}

constexpr uint16_t kObject = 0x0102;

// fec_id 5: an item is fec_id, 0, object id, then block (24 bits) and symbol (8 bits), big-endian
void put_item(std::vector<uint8_t>& out, uint16_t obj, uint32_t block, uint32_t symbol, uint8_t fec_id = 5)
{
    const uint8_t b[8] = {fec_id, 0, (uint8_t)(obj >> 8), (uint8_t)obj, (uint8_t)(block >> 16), (uint8_t)(block >> 8), (uint8_t)block,
                          (uint8_t)symbol};
    out.insert(out.end(), b, b + 8);
}
void put_request(std::vector<uint8_t>& out, uint8_t form, uint8_t flags, const std::vector<uint32_t>& block_symbol,
                 uint16_t obj = kObject)
{
    const size_t len = block_symbol.size() / 2 * 8;
    const uint8_t h[4] = {form, flags, (uint8_t)(len >> 8), (uint8_t)len};
    out.insert(out.end(), h, h + 4);
    for (size_t i = 0; i + 1 < block_symbol.size(); i += 2) put_item(out, obj, block_symbol[i], block_symbol[i + 1]);
}

// A receiver and a sender of nblocks blocks of k + m slots whose arrays each end their allocation,
// and a wire buffer that is open only where its messages lie.
struct Bench {
    uint32_t k, m, nblocks, stride, bwords;
    size_t cap;
    Arena a_mask, a_repair, a_block, a_object, a_trepair, a_tparity, a_tblock, a_tobject, a_nd, a_totals, a_pend, a_content, a_rows,
        a_wire, a_off, a_len;
    uint32_t* mask;
    nfec_rx_repair_state rx;
    nfec_tx_repair_state tx;
    uint16_t* nd;
    uint64_t* totals;
    uint32_t* pending_blocks;
    uint8_t* content;
    uint64_t* rows;
    nfec_rx_messages msgs;
    Bench(uint32_t k_, uint32_t m_, uint32_t nb)
        : k(k_), m(m_), nblocks(nb), stride((k_ + m_ + 31) / 32), bwords((nb + 31) / 32),
          cap((size_t)nb * ((k_ + m_ + 1) / 2) * 20 + 20), a_mask(nb * stride * 4), a_repair(nb * stride * 4), a_block(bwords * 4),
          a_object(4), a_trepair(nb * stride * 4), a_tparity(nb * 4), a_tblock(bwords * 4), a_tobject(4), a_nd(nb * 2), a_totals(48),
          a_pend(bwords * 4), a_content(cap), a_rows(((size_t)nb + 1) * 16), a_wire(1 << 18), a_off(8 * 4096), a_len(2 * 4096)
    {
        mask = a_mask.tail<uint32_t>((size_t)nb * stride);
        rx.repair = a_repair.tail<uint32_t>((size_t)nb * stride);
        rx.block_repair = a_block.tail<uint32_t>(bwords);
        rx.object = a_object.tail<uint32_t>(1);
        tx.repair = a_trepair.tail<uint32_t>((size_t)nb * stride);
        tx.parity = a_tparity.tail<uint16_t>((size_t)nb * 2);
        tx.block_repair = a_tblock.tail<uint32_t>(bwords);
        tx.object = a_tobject.tail<uint32_t>(1);
        nd = a_nd.tail<uint16_t>(nb);
        totals = a_totals.tail<uint64_t>(6);
        pending_blocks = a_pend.tail<uint32_t>(bwords);
        content = a_content.tail<uint8_t>(cap);
        rows = a_rows.tail<uint64_t>(((size_t)nb + 1) * 2);
        std::memset(mask, 0, (size_t)nb * stride * 4);
        std::memset(tx.repair, 0, (size_t)nb * stride * 4);
        std::memset(tx.parity, 0, (size_t)nb * 4);
        std::memset(tx.block_repair, 0, bwords * 4);
        *tx.object = 0;
        for (uint32_t b = 0; b < nb; ++b) nd[b] = (uint16_t)k;
        zero_rx();
        std::memset(&msgs, 0, sizeof msgs);
    }
    void zero_rx()  // the start of a NACK cycle
    {
        std::memset(rx.repair, 0, (size_t)nblocks * stride * 4);
        std::memset(rx.block_repair, 0, bwords * 4);
        *rx.object = 0;
    }
    // the messages into the wire buffer, each ending on an 8-byte boundary with a closed granule behind it
    void load(const std::vector<std::vector<uint8_t>>& messages)
    {
        a_wire.open_all();
        uint64_t* off = a_off.tail<uint64_t>(messages.size());
        uint16_t* len = a_len.tail<uint16_t>(messages.size());
        size_t at = 64;
        std::vector<std::pair<size_t, size_t>> open;
        for (size_t i = 0; i < messages.size(); ++i) {
            const size_t n = messages[i].size();
            size_t end = (at + n + 7) & ~(size_t)7;
            if (n) std::memcpy(a_wire.p + end - n, messages[i].data(), n);
            off[i] = end - n, len[i] = (uint16_t)n;
            open.push_back({end - n, n});
            at = end + 16;
        }
        a_wire.close();
        for (auto& r : open) a_wire.open(a_wire.p + r.first, r.second);
        msgs.payloads = a_wire.p, msgs.payload_bytes = at;
        msgs.offsets = off, msgs.length = len, msgs.count = (uint32_t)messages.size(), msgs.count_dev = nullptr;
    }
    int handle() { return nfec_rx_handle_repair_content_host(k, m, &msgs, 5, 8, kObject, 0, mask, stride, nd, nblocks, &rx, totals); }
    int decide(uint32_t flags) { return nfec_rx_repair_pending_host(k, m, mask, stride, nd, nblocks, &rx, flags, pending_blocks, totals); }
    // this receiver's own NACK content
    std::vector<uint8_t> nack(uint32_t flags, uint32_t max_units)
    {
        if (nfec_rx_repair_requests_host(k, m, mask, stride, nd, nblocks, 5, 8, kObject, 0, flags, max_units, content, cap, rows,
                                         totals) != NFEC_OK)
            fail_case("nack rc", 0, 0);
        if (totals[0] > cap || totals[0] > 60000) fail_case("nack size", totals[0], cap);
        return std::vector<uint8_t>(content, content + std::min<uint64_t>(totals[0], cap));
    }
    std::vector<uint8_t> adv(uint32_t max_units, uint64_t capacity)
    {
        if (nfec_tx_repair_adv_host(k, m, &tx, stride, nd, nblocks, 5, 8, kObject, 0, max_units, content + (cap - capacity), capacity,
                                    rows, totals) != NFEC_OK)
            fail_case("adv rc", 0, 0);
        const uint8_t* at = content + (cap - capacity);
        return std::vector<uint8_t>(at, at + std::min<uint64_t>(totals[0], capacity));
    }
    void random_mask(uint64_t& seed, uint32_t loss_percent)
    {
        for (uint32_t b = 0; b < nblocks; ++b) {
            const uint32_t kind = rnd(seed) % 8;
            for (uint32_t w = 0; w < stride; ++w) mask[(size_t)b * stride + w] = 0;
            for (uint32_t s = 0; s < stride * 32; ++s) {  // (bits past nd + m are noise: they are ignored)
                const bool got = kind == 0 ? false : kind == 1 ? s < k || s >= (uint32_t)nd[b] + m : rnd(seed) % 100 >= loss_percent;
                if (got && !(kind == 0 && s < (uint32_t)nd[b] + m)) mask[(size_t)b * stride + (s >> 5)] |= 1u << (s & 31u);
            }
        }
    }
};

std::vector<std::vector<uint8_t>> split(const std::vector<uint8_t>& content, size_t limit)
{
    std::vector<std::vector<uint8_t>> out;
    size_t at = 0, start = 0;
    while (at + 4 <= content.size()) {
        const size_t size = 4 + ((size_t)content[at + 2] << 8 | content[at + 3]);
        if (at + size - start > limit && at > start) {
            out.emplace_back(content.begin() + start, content.begin() + at);
            start = at;
        }
        at += size;
    }
    if (content.size() > start) out.emplace_back(content.begin() + start, content.end());
    return out;
}

void self_suppression()
{
    uint64_t seed = 3;
    for (uint32_t trial = 0; trial < 60; ++trial) {
        const uint32_t k = trial % 3 == 0 ? 3 : trial % 3 == 1 ? 8 : 64, m = k / 2 + 1, nb = 1 + rnd(seed) % 70;
        Bench s(k, m, nb);
        for (uint32_t b = 0; b < nb; ++b)
            if (rnd(seed) % 7 == 0) s.nd[b] = (uint16_t)(rnd(seed) % (k + 2));
        s.random_mask(seed, 20 + 25 * (trial % 3));
        const uint32_t flags = trial & 1u;
        const std::vector<uint8_t> own = s.nack(flags, 1 + rnd(seed) % 40);
        const uint64_t needing = s.totals[2], absent = s.totals[3];
        // nothing heard: every needing and absent block is pending
        if (s.decide(flags) != NFEC_OK || s.totals[1] != needing + absent || s.totals[0] != (flags || needing + absent ? 1u : 0u))
            fail_case("nothing heard", trial, s.totals[1]);
        s.load(split(own, 200));
        if (s.handle() != NFEC_OK || s.totals[4] || s.totals[5]) fail_case("own nack rc", trial, s.totals[4]);
        std::vector<uint32_t> rep(s.rx.repair, s.rx.repair + (size_t)nb * s.stride);
        if (s.decide(flags) != NFEC_OK || s.totals[0] != 0 || s.totals[1] != 0 || s.totals[2] != needing || s.totals[3] != absent)
            fail_case("self-suppression", trial, s.totals[1]);
        if (std::memcmp(rep.data(), s.rx.repair, rep.size() * 4)) fail_case("the decision changed the state", trial, 0);
        for (uint32_t w = 0; w < s.bwords; ++w)
            if (s.pending_blocks[w]) fail_case("pending word", trial, w);
        // no bit at or past nd + m
        for (uint32_t b = 0; b < nb; ++b) {
            const uint32_t n = s.nd[b] >= 1 && s.nd[b] <= k ? s.nd[b] + m : 0;
            for (uint32_t t = n; t < s.stride * 32; ++t)
                if ((s.rx.repair[(size_t)b * s.stride + (t >> 5)] >> (t & 31u)) & 1u) fail_case("bit past nd + m", trial, b);
        }
        // the sender that handled the NACK advertises it: the advertisement is well-formed and a
        // fresh receiver with the same reception takes every unit of it that names a held block
        nfec_rx_messages one = s.msgs;
        uint64_t t6[6];
        if (nfec_tx_handle_nacks_host(k, m, &one, 5, 8, kObject, 0, s.nd, nb, s.stride, 0, &s.tx, 1u << 20, t6) != NFEC_OK)
            fail_case("tx handle rc", trial, 0);
        const std::vector<uint8_t> advertised = s.adv(1 + rnd(seed) % 40, s.cap);
        const uint64_t adv_total = s.totals[0];
        const uint64_t adv_requests = s.totals[1];
        for (uint64_t capacity : {(uint64_t)0, (uint64_t)5, adv_total / 2 + 1, adv_total}) {  // capacity cuts: the totals stand
            s.adv(1u << 10, std::min<uint64_t>(capacity, s.cap));
            if (s.totals[0] > adv_total || s.totals[1] > adv_requests) fail_case("adv totals under a capacity", trial, s.totals[0]);
        }
        s.zero_rx();
        s.load(split(advertised, 1400));
        if (s.handle() != NFEC_OK || s.totals[4] || s.totals[5] || s.totals[2] > s.totals[0]) fail_case("adv handled", trial, s.totals[4]);
        if (((*s.tx.object & NFEC_TX_REPAIR_INFO) != 0) != ((*s.rx.object & NFEC_RX_REPAIR_INFO) != 0) && adv_total)
            fail_case("adv INFO", trial, *s.rx.object);
    }
}

void order_and_split()
{
    uint64_t seed = 17;
    for (uint32_t trial = 0; trial < 40; ++trial) {
        const uint32_t k = 8, m = 4, nb = 40;
        Bench s(k, m, nb);
        s.random_mask(seed, 45);
        std::vector<std::vector<uint8_t>> messages(2 + rnd(seed) % 6);
        for (auto& msg : messages)
            for (uint32_t r = 1 + rnd(seed) % 4; r-- > 0;) {
                const uint8_t form = rnd(seed) % 2 ? REPAIR_RANGES : REPAIR_ITEMS;
                const uint8_t flags = (uint8_t)((rnd(seed) % 3 ? REPAIR_SEGMENT : REPAIR_BLOCK) | (rnd(seed) % 5 ? 0 : REPAIR_INFO));
                std::vector<uint32_t> items;
                for (uint32_t i = (1 + rnd(seed) % 3) * (form == REPAIR_RANGES ? 2 : 1); i-- > 0;)
                    items.push_back(rnd(seed) % (nb + 2)), items.push_back(rnd(seed) % (k + m + 3));
                put_request(msg, form, flags, items);
            }
        s.load(messages);
        s.handle();
        std::vector<uint32_t> rep(s.rx.repair, s.rx.repair + (size_t)nb * s.stride), blk(s.rx.block_repair, s.rx.block_repair + s.bwords);
        const uint32_t word = *s.rx.object;
        s.zero_rx();
        std::reverse(messages.begin(), messages.end());
        const size_t half = messages.size() / 2;
        s.load(std::vector<std::vector<uint8_t>>(messages.begin(), messages.begin() + half));
        s.handle();
        s.load(std::vector<std::vector<uint8_t>>(messages.begin() + half, messages.end()));
        s.handle();
        if (std::memcmp(rep.data(), s.rx.repair, rep.size() * 4) || std::memcmp(blk.data(), s.rx.block_repair, blk.size() * 4) ||
            word != *s.rx.object)
            fail_case("order or split changed the state", trial, 0);
    }
}

// random content, some of it damaged; the sanitizers are the check
void fuzz()
{
    uint64_t seed = 11;
    for (uint32_t trial = 0; trial < 300; ++trial) {
        const uint32_t k = trial % 3 == 0 ? 3 : trial % 3 == 1 ? 8 : 64, m = k / 2 + 1, nb = 1 + rnd(seed) % 40;
        Bench s(k, m, nb);
        for (uint32_t b = 0; b < nb; ++b)
            if (rnd(seed) % 7 == 0) s.nd[b] = (uint16_t)(rnd(seed) % (k + 2));
        s.random_mask(seed, 10 + 20 * (trial % 4));
        std::vector<std::vector<uint8_t>> messages(1 + rnd(seed) % 6);
        for (auto& msg : messages) {
            for (uint32_t r = rnd(seed) % 5; r-- > 0;) {
                const uint8_t form = rnd(seed) % 2 ? REPAIR_RANGES : REPAIR_ITEMS;
                const uint8_t flags = (uint8_t)(rnd(seed) % 10 == 0 ? rnd(seed) % 16 : rnd(seed) % 4 ? REPAIR_SEGMENT : REPAIR_BLOCK);
                std::vector<uint32_t> items;
                for (uint32_t i = (1 + rnd(seed) % 4) * (form == REPAIR_RANGES ? 2 : 1); i-- > 0;) {
                    items.push_back(rnd(seed) % 9 ? rnd(seed) % (nb + 2) : rnd(seed) & 0xffffffu);
                    items.push_back(rnd(seed) % (k + m + 3));
                }
                put_request(msg, form, flags, items, rnd(seed) % 11 ? kObject : (uint16_t)rnd(seed));
            }
            const uint32_t damage = rnd(seed) % 8;
            if (damage == 0 && msg.size() > 3) msg.resize(msg.size() - 1 - rnd(seed) % 3);
            if (damage == 1 && msg.size() > 3) msg[2] = 0xff;
            if (damage == 2 && msg.size() > 4) msg[4 + 8 * (rnd(seed) % ((msg.size() - 4) / 8 + 1)) % (msg.size() - 4)] ^= 7;
        }
        s.load(messages);
        if (s.handle() != NFEC_OK) fail_case("fuzz rc", trial, 0);
        if (s.totals[1] + s.totals[2] > s.totals[0]) fail_case("fuzz totals", trial, s.totals[0]);
        uint64_t bits = 0;
        for (uint32_t b = 0; b < nb; ++b) bits += (s.rx.block_repair[b >> 5] >> (b & 31u)) & 1u;
        if (bits != s.totals[3]) fail_case("fuzz newly set", bits, s.totals[3]);
        for (uint32_t b = nb; b < s.bwords * 32; ++b)
            if ((s.rx.block_repair[b >> 5] >> (b & 31u)) & 1u) fail_case("fuzz block bit past nblocks", trial, b);
        for (uint32_t b = 0; b < nb; ++b) {
            const uint32_t n = s.nd[b] >= 1 && s.nd[b] <= k ? s.nd[b] + m : 0;
            for (uint32_t t = n; t < s.stride * 32; ++t)
                if ((s.rx.repair[(size_t)b * s.stride + (t >> 5)] >> (t & 31u)) & 1u) fail_case("fuzz bit past nd + m", trial, b);
        }
        std::memset(s.pending_blocks, 0xff, s.bwords * 4);  // the caller does not zero it
        if (s.decide(trial & 1u) != NFEC_OK) fail_case("fuzz decide rc", trial, 0);
        uint64_t pend = 0;
        for (uint32_t b = 0; b < s.bwords * 32; ++b) {
            const bool p = (s.pending_blocks[b >> 5] >> (b & 31u)) & 1u;
            if (p && b >= nb) fail_case("fuzz pending bit past nblocks", trial, b);
            pend += p;
        }
        if (pend != s.totals[1]) fail_case("fuzz pending count", pend, s.totals[1]);
        // the advertisement of a sender state made of the same noise
        for (uint32_t i = 0; i < nb * s.stride; ++i) s.tx.repair[i] = rnd(seed) & rnd(seed);
        for (uint32_t w = 0; w < s.bwords; ++w) s.tx.block_repair[w] = rnd(seed) & rnd(seed);
        *s.tx.object = rnd(seed) % 8 == 0 ? NFEC_TX_REPAIR_OBJECT : rnd(seed) % 4 * 2;
        const std::vector<uint8_t> advertised = s.adv(1 + rnd(seed) % 30, s.cap);
        const uint64_t full = s.totals[0];
        s.adv(1 + rnd(seed) % 30, full ? rnd(seed) % full : 0);  // a capacity that cuts it anywhere
        uint64_t consumed = 0;
        const int units = nfec_repair_parse_host(5, 8, advertised.data(), advertised.size(), nullptr, nullptr, nullptr, nullptr, 0, &consumed);
        if (units < 0 || consumed != advertised.size()) fail_case("fuzz adv does not parse", trial, consumed);
    }
}

void unreadable()
{
    Bench s(8, 4, 2);
    s.mask[0] = s.mask[1] = 1;  // needing
    std::vector<uint8_t> good;
    put_request(good, REPAIR_ITEMS, REPAIR_SEGMENT, {0, 8, 1, 9});
    s.load({good, good, good});
    uint64_t* off = const_cast<uint64_t*>(s.msgs.offsets);
    off[1] = s.msgs.payload_bytes - 4;  // reaches past the end: no byte of it may be loaded
    off[2] = ~0ull;
    if (s.handle() != NFEC_OK || s.totals[0] != 2 || s.totals[1] != 2 || s.totals[5] != 2) fail_case("unreadable", s.totals[0], s.totals[5]);
}

}  // namespace

int main()
{
    self_suppression();
    order_and_split();
    fuzz();
    unreadable();
    if (failures) {
        std::printf("%d cases failed\n", failures);
        return 1;
    }
    std::printf("suppress driver done\n");
    return 0;
}
