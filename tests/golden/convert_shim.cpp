// convert_shim.cpp -- C entry points around the reference's two converters (lib_rspt/lib_signalpacker/utils.h:
// convert_native_to_i32, convert_i32_to_native) and its four packers, for tests/golden/make_convert_record.py.  The reference's
// headers are included from where they lie and its sources are compiled beside this file by the generator; nothing of them is
// restated here.  planar is a contiguous [nch][ns] int32 matrix; the reference takes one pointer per channel.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "lib_rspt/signal_packer.h"
#include "lib_rspt/lib_signalpacker/utils.h"

namespace {
std::vector<int32_t*> rows_of(int32_t* planar, int nch, int ns) {
    std::vector<int32_t*> r((size_t)nch);
    for (int c = 0; c < nch; ++c) r[(size_t)c] = planar + (size_t)c * ns;
    return r;
}
}  // namespace

extern "C" void convert_shim_native_to_i32(int32_t* planar, const uint8_t* native, int ns, int nch, int bps, int reverse) {
    std::vector<int32_t*> r = rows_of(planar, nch, ns);
    convert_native_to_i32(r.data(), native, ns, nch, bps, reverse != 0);
}

extern "C" void convert_shim_i32_to_native(uint8_t* native, int32_t* planar, int ns, int nch, int bps, int reverse) {
    std::vector<int32_t*> r = rows_of(planar, nch, ns);
    convert_i32_to_native(native, r.data(), ns, nch, bps, reverse != 0);
}

// kind: the numbering of include/rspt_hip.h (0 hzr, 1 xdelta_hzr, 2 dct, 3 hadamard); returns the stream's length
extern "C" size_t convert_shim_pack(int kind, const uint8_t* src, size_t bps, size_t nch, size_t ns, size_t nb, uint8_t* dst, size_t cap) {
    i_signal_packer* p = kind == 0   ? i_signal_packer::new_hzr(bps, nch, ns)
                         : kind == 1 ? i_signal_packer::new_xdelta_hzr(bps, nch, ns, nb)
                         : kind == 2 ? i_signal_packer::new_dct(bps, nch, ns)
                                     : i_signal_packer::new_hadamard(bps, nch, ns);
    size_t n = 0;
    p->compress(src, dst, cap, n);
    if (kind == 0) i_signal_packer::delete_hzr(p);
    else if (kind == 1) i_signal_packer::delete_xdelta_hzr(p);
    else if (kind == 2) i_signal_packer::delete_dct(p);
    else i_signal_packer::delete_hadamard(p);
    return n;
}
