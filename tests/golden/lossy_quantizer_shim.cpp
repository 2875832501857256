/*
 * lossy_quantizer_shim.cpp -- C entry point around the reference's dct and hadamard packers for
 * tests/golden/make_lossy_quantizer_record.py.  TEST INFRASTRUCTURE ONLY: this file is ours and holds no reference code.  The
 * generator compiles it with the reference's sources, two of them patched in its temporary build directory so that their
 * `quality` and nr_bytes_to_compress_ constants can be chosen per packer instance.
 *
 * One call is one packer life: construct, compress, decompress, destroy (i_signal_packer, lib_rspt/signal_packer.h:29-73).
 */
#include <cstddef>
#include <cstdint>

#include "signal_packer.h"

extern "C" int lossy_quantizer_shim_roundtrip(int kind, const uint8_t* src, size_t bps, size_t nch, size_t ns, uint8_t* stream, size_t stream_cap,
                                              size_t* stream_len, uint8_t* decoded, size_t* consumed) {
    i_signal_packer* p = kind == 2 ? i_signal_packer::new_dct(bps, nch, ns) : kind == 3 ? i_signal_packer::new_hadamard(bps, nch, ns) : nullptr;
    if (!p) return -1;
    size_t len = 0, used = 0;
    p->compress(src, stream, stream_cap, len);
    const int rc = p->decompress(stream, used, decoded);
    *stream_len = len;
    *consumed = used;
    if (kind == 2)
        i_signal_packer::delete_dct(p);
    else
        i_signal_packer::delete_hadamard(p);
    return rc;
}
