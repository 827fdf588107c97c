// tx_repair_asan.cpp -- the sender's repair state on the host (norm_amd/csrc/tx_repair_host.cpp over
// the rule of repair_layout.hpp: nfec_tx_handle_nacks_host, nfec_tx_activate_repairs_host and
// nfec_tx_end_blocks_host) under AddressSanitizer and UBSan, with every byte a call may not touch
// poisoned: the wire buffer is closed except for the messages themselves (each ends on an 8-byte
// boundary, so the byte behind it is closed exactly), and the four state arrays, the pending mask,
// numData and the totals each end their allocation.  (The host entries take no workspace; the
// device entry's is sized by nfec_tx_nack_workspace_bytes and checked on the device.)  What is
// checked besides the sanitizers' silence: the "order decides" pair of nfec.h's rule, that a call
// whose units exceed the capacity changes no byte of the state, that damaged and unreadable
// messages are counted, and that activation and the end-of-block step leave bits at or past nd + m
// alone.  Host code only, no GPU; `make -C tests/native -f tx_repair_asan.mk`.
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nfec.h"
#include "repair_layout.hpp"

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

// A sender of nblocks blocks of k + m slots whose arrays each end their allocation, and a wire
// buffer that is open only where its messages lie.
struct Bench {
    uint32_t k, m, nblocks, stride;
    Arena a_repair, a_parity, a_block, a_object, a_pending, a_nd, a_totals, a_wire, a_off, a_len;
    nfec_tx_repair_state st;
    uint32_t* pending;
    uint16_t* nd;
    uint64_t* totals;
    nfec_rx_messages msgs;
    Bench(uint32_t k_, uint32_t m_, uint32_t nb, uint32_t parity_offset)
        : k(k_), m(m_), nblocks(nb), stride((k_ + m_ + 31) / 32), a_repair(nb * stride * 4), a_parity(nb * 4),
          a_block((nb + 31) / 32 * 4), a_object(4), a_pending(nb * stride * 4), a_nd(nb * 2), a_totals(48), a_wire(1 << 18),
          a_off(8 * 4096), a_len(2 * 4096)
    {
        st.repair = a_repair.tail<uint32_t>((size_t)nb * stride);
        st.parity = a_parity.tail<uint16_t>((size_t)nb * 2);
        st.block_repair = a_block.tail<uint32_t>((nb + 31) / 32);
        st.object = a_object.tail<uint32_t>(1);
        pending = a_pending.tail<uint32_t>((size_t)nb * stride);
        nd = a_nd.tail<uint16_t>(nb);
        totals = a_totals.tail<uint64_t>(6);
        std::memset(st.repair, 0, (size_t)nb * stride * 4);
        std::memset(st.block_repair, 0, (nb + 31) / 32 * 4);
        std::memset(pending, 0, (size_t)nb * stride * 4);
        *st.object = 0;
        for (uint32_t b = 0; b < nb; ++b) st.parity[2 * b] = (uint16_t)parity_offset, st.parity[2 * b + 1] = 0, nd[b] = (uint16_t)k;
        std::memset(&msgs, 0, sizeof msgs);
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
    int handle(uint32_t extra, uint32_t capacity)
    {
        return nfec_tx_handle_nacks_host(k, m, &msgs, 5, 8, kObject, 0, nd, nblocks, stride, extra, &st, capacity, totals);
    }
    bool bit(uint32_t b, uint32_t s) const { return (st.repair[(size_t)b * stride + (s >> 5)] >> (s & 31u)) & 1u; }
};

void order_decides()
{
    // k = 8, m = 4, parity {1, 0}: A = RANGES (8, 12), B = RANGES (8, 10)
    std::vector<uint8_t> A, B;
    put_request(A, REPAIR_RANGES, REPAIR_SEGMENT, {0, 8, 0, 12});
    put_request(B, REPAIR_RANGES, REPAIR_SEGMENT, {0, 8, 0, 10});
    for (int order = 0; order < 2; ++order) {
        Bench s(8, 4, 1, 1);
        s.load(order ? std::vector<std::vector<uint8_t>>{B, A} : std::vector<std::vector<uint8_t>>{A, B});
        if (s.handle(0, 16) != NFEC_OK) fail_case("order rc", order, 0);
        uint32_t bits = 0;
        for (uint32_t t = 0; t < 12; ++t) bits |= (uint32_t)s.bit(0, t) << t;
        if (bits != (order ? 0xF00u : 0xE00u)) fail_case("order bits", order, bits);
        if (s.totals[0] != 2 || s.totals[1] != 2) fail_case("order totals", s.totals[0], s.totals[1]);
    }
}

// random content, some of it damaged; the sanitizers are the check
void fuzz()
{
    uint64_t seed = 11;
    for (uint32_t trial = 0; trial < 300; ++trial) {
        const uint32_t k = trial % 3 == 0 ? 3 : trial % 3 == 1 ? 8 : 64, m = k / 2 + 1, nb = 1 + rnd(seed) % 40;
        Bench s(k, m, nb, rnd(seed) % (m + 1));
        for (uint32_t b = 0; b < nb; ++b)
            if (rnd(seed) % 7 == 0) s.nd[b] = (uint16_t)(rnd(seed) % (k + 2));
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
        std::vector<uint32_t> repair0(s.st.repair, s.st.repair + (size_t)nb * s.stride);
        std::vector<uint16_t> parity0(s.st.parity, s.st.parity + 2 * nb);
        // the count first: a capacity of 0 changes nothing
        if (s.handle(trial % 3, 0) != NFEC_OK) fail_case("fuzz rc", trial, 0);
        const uint64_t units = s.totals[0];
        if (units && (std::memcmp(repair0.data(), s.st.repair, repair0.size() * 4) || std::memcmp(parity0.data(), s.st.parity, nb * 4) ||
                      *s.st.object || s.totals[1] || s.totals[3]))
            fail_case("fuzz overflow changed the state", trial, units);
        if (units > 1) {
            s.handle(trial % 3, (uint32_t)units - 1);
            if (std::memcmp(repair0.data(), s.st.repair, repair0.size() * 4)) fail_case("fuzz one too few", trial, units);
        }
        if (s.handle(trial % 3, (uint32_t)units) != NFEC_OK || s.totals[0] != units) fail_case("fuzz units", trial, units);
        if (s.totals[1] + s.totals[2] > units) fail_case("fuzz totals", trial, units);
        // no bit at or past nd + m, in the repair mask and behind activation in the pending mask
        uint64_t act[3];
        const uint32_t auto_parity = trial % (m + 1);
        if (nfec_tx_activate_repairs_host(k, m, s.nd, nb, auto_parity, s.pending, s.stride, &s.st, act) != NFEC_OK)
            fail_case("fuzz activate rc", trial, 0);
        uint64_t bits = 0;
        for (uint32_t b = 0; b < nb; ++b) {
            const uint32_t n = s.nd[b] >= 1 && s.nd[b] <= k ? s.nd[b] + m : 0;
            for (uint32_t t = 0; t < s.stride * 32; ++t) {
                const bool p = (s.pending[(size_t)b * s.stride + (t >> 5)] >> (t & 31u)) & 1u;
                if (t >= n && (p || s.bit(b, t))) fail_case("fuzz bit past nd + m", trial, b);
                if (t < n && s.bit(b, t)) fail_case("fuzz repair left behind activation", trial, b);
                bits += p;
            }
        }
        if (bits != act[2]) fail_case("fuzz pending bits", bits, act[2]);
        if (*s.st.object & ~(uint32_t)TXR_PENDING_INFO) fail_case("fuzz object word", trial, *s.st.object);
        // the end of block, twice: idempotent
        std::memset(s.pending, 0, (size_t)nb * s.stride * 4);
        nfec_tx_end_blocks_host(k, m, s.nd, nb, s.pending, s.stride, &s.st);
        std::vector<uint16_t> once(s.st.parity, s.st.parity + 2 * nb);
        nfec_tx_end_blocks_host(k, m, s.nd, nb, s.pending, s.stride, &s.st);
        if (std::memcmp(once.data(), s.st.parity, nb * 4)) fail_case("fuzz end_blocks twice", trial, 0);
        for (uint32_t b = 0; b < nb; ++b)
            if (s.nd[b] >= 1 && s.nd[b] <= k && (s.st.parity[2 * b] > m || s.st.parity[2 * b + 1])) fail_case("fuzz parity pair", trial, b);
    }
}

void unreadable()
{
    Bench s(8, 4, 2, 0);
    std::vector<uint8_t> good;
    put_request(good, REPAIR_ITEMS, REPAIR_SEGMENT, {0, 8, 1, 9});
    s.load({good, good, good});
    uint64_t* off = const_cast<uint64_t*>(s.msgs.offsets);
    off[1] = s.msgs.payload_bytes - 4;  // reaches past the end: no byte of it may be loaded
    off[2] = ~0ull;
    if (s.handle(0, 16) != NFEC_OK || s.totals[0] != 2 || s.totals[5] != 2) fail_case("unreadable", s.totals[0], s.totals[5]);
}

}  // namespace

int main()
{
    order_decides();
    fuzz();
    unreadable();
    if (failures) {
        std::printf("%d cases failed\n", failures);
        return 1;
    }
    std::printf("tx repair driver done\n");
    return 0;
}
