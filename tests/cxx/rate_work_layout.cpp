// rate_work_layout.cpp -- the work-area layouts of the rate-control entries (rspt_amd/csrc/rate_work.hpp), swept on the CPU.
// Built with -fsanitize=address,undefined and run by tests/test_rate_work_layout.py; prints the number of layouts checked.
//
// For every layout: each part starts on a 256-byte boundary, the parts lie one behind the other inside `bytes`, and `bytes` is the
// figure stated here a second time, from the sizes alone.  Small layouts are put onto a heap block of exactly `bytes` and every
// part is written in full, under the sanitizer's eyes.  A null base is never offset: it has no parts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../rspt_amd/csrc/rate_work.hpp"

using namespace rate_work;

static long checked = 0;

#define REQUIRE(cond)                                                                                             \
    do {                                                                                                          \
        if (!(cond)) {                                                                                            \
            std::fprintf(stderr, "%s:%d: %s\n  %s\n", __FILE__, __LINE__, #cond, what);                           \
            std::exit(1);                                                                                         \
        }                                                                                                         \
    } while (0)

struct Part {
    size_t at, size;
};

// parts in the order they lie in an area of `bytes`; the area is written through part() where it is small
static void holds(const std::vector<Part>& parts, size_t bytes, const char* what) {
    size_t end = 0;
    for (const Part& q : parts) {
        REQUIRE(q.at != kNone && q.at % 256 == 0);
        REQUIRE(q.at >= end);
        end = q.at + q.size;
        REQUIRE(end >= q.at && end <= bytes);
    }
    if (bytes <= (1u << 16)) {
        void* base = std::malloc(bytes);
        REQUIRE(base != nullptr);
        for (const Part& q : parts) std::memset(part<uint8_t>(base, q.at), 0x5a, q.size);
        std::free(base);
    }
    ++checked;
}

static std::vector<Part> tables(const Tables& t, size_t c, size_t base) {
    return {{base + t.prdn, 8 * c}, {base + t.mse, 8 * c}, {base + t.path, 4 * c}, {base + t.acc, 32 * c}, {base + t.flag, 4 * c}};
}

static std::vector<Part> scratch(const Target& t, size_t copy_bytes, size_t nz_bytes, size_t base) {
    std::vector<Part> v;
    if (t.orig != kNone) v.push_back({base + t.orig, copy_bytes});
    if (t.dec != kNone) v.push_back({base + t.dec, copy_bytes});
    if (t.nz != kNone) v.push_back({base + t.nz, nz_bytes});
    return v;
}

static void append(std::vector<Part>& v, const std::vector<Part>& w) { v.insert(v.end(), w.begin(), w.end()); }

static void one(size_t N, size_t nblk, size_t bps, size_t B, size_t K) {
    char what[160];
    std::snprintf(what, sizeof what, "N %zu nblk %zu bps %zu nblocks %zu nladder %zu", N, nblk, bps, B, K);
    const size_t c = K * B, copy = pad(B * N * 4), nz = pad(B * 4 * nblk * 4);
    const size_t tab = 2 * pad(8 * c) + 2 * pad(4 * c) + pad(32 * c);
    const size_t cut = bps < 4 ? copy : 0;  // a planar form's orig: the matrix cut to the sample width

    const Tables t(c);
    REQUIRE(t.bytes == tab);
    holds(tables(t, c, 0), tab, what);
    REQUIRE(Tables(8 * B).bytes >= tab);  // Workspace::target_tab, sized for a full ladder, holds any ladder's

    for (Form form : {NATIVE, PLANAR_GENERAL, PLANAR_FUSED}) {
        const Target w(N, nblk, bps, B, K, form);
        const size_t want_scratch = form == NATIVE ? 2 * copy + nz : form == PLANAR_GENERAL ? cut + copy + nz : 0;
        REQUIRE(w.scratch == want_scratch);
        REQUIRE(w.bytes == (form == NATIVE ? 2 * copy + nz + tab : form == PLANAR_GENERAL ? (cut + copy + nz < 16 ? 16 : cut + copy + nz) : 16));
        REQUIRE((w.orig != kNone) == (form == NATIVE || (form == PLANAR_GENERAL && bps < 4)) && (w.dec != kNone) == (form != PLANAR_FUSED) &&
                (w.nz != kNone) == (form != PLANAR_FUSED));
        std::vector<Part> parts = scratch(w, B * N * 4, B * 4 * nblk * 4, 0);
        if (form == NATIVE) append(parts, tables(w.tab, c, w.scratch));  // a planar form's tables lie in the workspace, from 0 on
        REQUIRE(form == NATIVE || (w.tab.prdn == 0 && w.tab.bytes == tab));
        holds(parts, w.bytes, what);
    }

    REQUIRE(budget_bytes(B, K) == pad(8 * c));
    holds({{0, 8 * c}}, budget_bytes(B, K), what);

    const size_t head = 2 * pad(8 * c) + 1280;
    for (int fused = 0; fused < 2; ++fused)
        for (int planar = 0; planar < 2; ++planar) {
            const Total w(N, nblk, bps, B, K, fused, planar);
            REQUIRE(w.head == head);
            REQUIRE(w.bytes == (fused ? head + tab : planar ? head + cut + copy + nz + tab : head + Target(N, nblk, bps, B, K, NATIVE).bytes));
            std::vector<Part> parts = {{w.sizes, 8 * c}, {w.figs, 8 * c}, {w.res, 24}, {w.res + kTotalSlots, kTotalResBytes - kTotalSlots}};
            append(parts, scratch(w.t, B * N * 4, B * 4 * nblk * 4, w.head));
            append(parts, tables(w.t.tab, c, w.tab));
            // (the slots lie behind res inside one padded part: only res itself starts on a boundary of the area's)
            REQUIRE(w.res % 256 == 0 && kTotalSlots % 256 == 0 && kTotalResBytes % 256 == 0);
            holds(parts, w.bytes, what);
        }
}

int main() {
    const char* what = "a null base";
    REQUIRE(part<uint8_t>(nullptr, 256) == nullptr && part<uint8_t>(nullptr, 0) == nullptr && part<uint8_t>(nullptr, kNone) == nullptr);
    unsigned char byte = 0;
    REQUIRE(part<uint8_t>(&byte, kNone) == nullptr && part<uint8_t>(&byte, 0) == &byte);
    REQUIRE(Tables(8).bytes == 5 * 256 && Tables(8, 512).flag == 512 + 4 * 256);

    const size_t Ns[] = {24, 25, 63, 64, 65, 300, 1000, 8192, 24576, 98304, 131072, (1u << 22) - 1, 1u << 22};
    const size_t Bs[] = {1, 3, 4096, 4097, 65535};
    for (size_t N : Ns)
        for (size_t nblk = 1; nblk <= 64; ++nblk)
            for (size_t bps = 1; bps <= 4; ++bps)
                for (size_t B : Bs)
                    for (size_t K = 1; K <= 8; ++K) one(N, nblk, bps, B, K);
    std::printf("%ld layouts hold\n", checked);
    return 0;
}
