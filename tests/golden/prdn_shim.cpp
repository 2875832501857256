// prdn_shim.cpp -- runs the reference's own test_packer_ (lib_rspt_test/rspt_test.cpp:58-112) for
// tests/golden/make_prdn_record.py and returns the PRDN[%] it prints.  The reference's file is included at build time (its
// main renamed), so the loop that computes the figure is the reference's own text, compiled as the reference compiles it.
//   prdn_shim_run     a packer whose decompress() hands back a given decoded block: PRDN of any pair of blocks
//   prdn_shim_packer  one of the reference's packers: its real round trip (test_packer_ leaves the decoded block in _decoded.bin
//                     in the working directory, which is why the generator runs inside its temporary build directory)
// The text behind "PRDN[%] = " is returned as printed with 17 significant digits, which identifies a finite double; the
// generator turns "inf" and "nan" / "-nan" into their bit patterns.
#include <stddef.h>
#include <stdint.h>

#include <iomanip>
#include <sstream>
#include <string>

#define main rspt_test_main_
#include "lib_rspt_test/rspt_test.cpp"
#undef main

namespace {

struct given_decoded : i_signal_packer {
    const unsigned char* dec;
    size_t len;
    void compress(const unsigned char*, unsigned char*, size_t, size_t& dst_len) override { dst_len = 1; }
    int decompress(const unsigned char*, size_t& src_len, unsigned char* dst) override {
        memcpy(dst, dec, len);
        src_len = 1;
        return 0;
    }
};

int run(i_signal_packer* pk, const uint8_t* orig, int ns, int nch, int bps, char* out, size_t cap) {
    std::ostringstream os;
    std::streambuf* keep = std::cout.rdbuf(os.rdbuf());
    const std::streamsize digits = std::cout.precision(17);  // (the precision belongs to cout, not to the buffer behind it)
    test_packer_(pk, ns, nch, const_cast<uint8_t*>(orig), bps);
    std::cout.precision(digits);
    std::cout.rdbuf(keep);
    const std::string s = os.str(), key = "PRDN[%] = ";
    const size_t at = s.rfind(key);
    if (at == std::string::npos) return -1;
    std::string v = s.substr(at + key.size());
    while (!v.empty() && (v.back() == '\n' || v.back() == '\r' || v.back() == ' ')) v.pop_back();
    if (v.size() + 1 > cap) return -2;
    memcpy(out, v.c_str(), v.size() + 1);
    return s.find("WARNING") != std::string::npos ? 1 : 0;
}

}  // namespace

extern "C" int prdn_shim_run(const uint8_t* orig, const uint8_t* dec, int ns, int nch, int bps, char* out, size_t cap) {
    given_decoded pk;
    pk.dec = dec;
    pk.len = (size_t)ns * nch * bps;
    return run(&pk, orig, ns, nch, bps, out, cap);
}

// kind: 2 dct, 3 hadamard (the numbering of include/rspt_hip.h)
extern "C" int prdn_shim_packer(int kind, const uint8_t* orig, int ns, int nch, int bps, char* out, size_t cap) {
    i_signal_packer* pk = kind == 2 ? i_signal_packer::new_dct(bps, nch, ns) : i_signal_packer::new_hadamard(bps, nch, ns);
    const int rc = run(pk, orig, ns, nch, bps, out, cap);
    if (kind == 2) i_signal_packer::delete_dct(pk);
    else i_signal_packer::delete_hadamard(pk);
    return rc;
}
