// rate_work.hpp -- where the parts of the rate-control entries' work areas lie (host_target.hip, host_budget.hip, host_total.hip).
//
// Plain C++ and no HIP: a layout is a set of byte OFFSETS computed from the plain numbers of a call -- N = nch * ns, nblk, bps,
// nblocks, nladder, the form and the route -- so that a sizing call needs no base, and tests/cxx/rate_work_layout.cpp checks every
// layout on the CPU.  A pointer appears only where part() puts an offset onto a base that is one.  Every part starts on a
// 256-byte boundary of its area.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rate_work {

constexpr size_t kNone = ~(size_t)0;  // the offset of a part that this form does not have
constexpr size_t pad(size_t n) { return (n + 255) & ~(size_t)255; }

template <class T>
inline T* part(void* base, size_t off) {
    return base && off != kNone ? reinterpret_cast<T*>(static_cast<uint8_t*>(base) + off) : nullptr;
}

// The five figure tables of cells = nladder * nblocks candidates, from `at` on:
//   prdn, mse [cells] double, path [cells] uint32: what the PRDN stage says of each candidate
//   acc [cells][4] uint64, flag [cells] uint32:    the fused probe's exact sums and k_q_finish's flags
struct Tables {
    size_t prdn, mse, path, acc, flag, bytes;
    constexpr explicit Tables(size_t cells, size_t at = 0)
        : prdn(at),
          mse(prdn + pad(cells * 8)),
          path(mse + pad(cells * 8)),
          acc(path + pad(cells * 4)),
          flag(acc + pad(cells * 32)),
          bytes(flag + pad(cells * 4) - at) {}
};

// The target entry.  NATIVE keeps everything in d_work; the planar forms keep the tables in the handle's workspace
// (Workspace::target_tab), so that their d_work holds block-sized scratch alone -- and at least 16 bytes, to be a pointer.
enum Form { NATIVE, PLANAR_GENERAL, PLANAR_FUSED };
struct Target {
    size_t orig = kNone, dec = kNone, nz = kNone;  // in d_work: two planar copies of the batch, the candidates' non-zero marks
    size_t scratch = 0;                            // bytes of those three
    Tables tab;                                    // from where the tables lie: d_work + scratch (NATIVE), or the workspace
    size_t bytes;                                  // of d_work
    constexpr Target(size_t N, size_t nblk, size_t bps, size_t nblocks, size_t nladder, Form form) : tab(nladder * nblocks), bytes(0) {
        const size_t copy = pad(nblocks * N * 4);
        if (form == NATIVE || (form == PLANAR_GENERAL && bps < 4)) orig = scratch, scratch += copy;
        if (form != PLANAR_FUSED) {
            dec = scratch, scratch += copy;
            nz = scratch, scratch += pad(nblocks * 4 * nblk * 4);
        }
        bytes = form == NATIVE ? scratch + tab.bytes : scratch < 16 ? 16 : scratch;
    }
};

// The budget entry, either form and route: the table of sizes, [nladder][nblocks] uint64.
constexpr size_t budget_bytes(size_t nblocks, size_t nladder) { return pad(nladder * nblocks * 8); }

// The total entry: a head -- sizes and figs, [nladder][nblocks] uint64 each, then res: three words and the rounds' slots behind
// them from kTotalSlots on -- then the target entry's block-sized scratch (the general route; none of it on the fused one, whose
// form is PLANAR_FUSED from either source), then the five tables.
constexpr size_t kTotalSlots = 256, kTotalResBytes = 1280;
struct Total {
    size_t sizes, figs, res, head;
    Target t;  // its offsets count from head
    size_t tab;  // where its tables lie
    size_t bytes;
    static constexpr Form form(bool fused, bool planar) { return fused ? PLANAR_FUSED : planar ? PLANAR_GENERAL : NATIVE; }
    constexpr Total(size_t N, size_t nblk, size_t bps, size_t nblocks, size_t nladder, bool fused, bool planar)
        : sizes(0),
          figs(pad(nladder * nblocks * 8)),
          res(2 * figs),
          head(res + kTotalResBytes),
          t(N, nblk, bps, nblocks, nladder, form(fused, planar)),
          tab(head + t.scratch),
          bytes(tab + t.tab.bytes) {}
};

}  // namespace rate_work
