// The body of k_fwht_cross, k_fwht_cross_q and k_fwht_cross_l (transforms.hip), included into each so that the quality-1 kernel stays the code
// that was timed.  From the kernel: planar, g, means, mean_i32, m, stride, last; QUANT (constexpr bool) and, where set, div.
    const uint32_t c = blockIdx.y, b = blockIdx.z, n = g.ns;
    int32_t* row = planar + (size_t)b * g.N + (size_t)c * n;
    const uint32_t col = blockIdx.x * 256u + threadIdx.x;  // < n / m
    const int32_t mean = !last ? 0 : FORWARD ? mean_i32[(size_t)b * g.nch + c] : load_mean_hdr(means, g, b, c);
    const uint32_t span = stride * m;
    switch (m) {
        case 2: fwht_cross_body<FORWARD, QUANT, 2>(row, col, stride, span, last != 0, n, mean, div); break;
        case 4: fwht_cross_body<FORWARD, QUANT, 4>(row, col, stride, span, last != 0, n, mean, div); break;
        case 8: fwht_cross_body<FORWARD, QUANT, 8>(row, col, stride, span, last != 0, n, mean, div); break;
        case 16: fwht_cross_body<FORWARD, QUANT, 16>(row, col, stride, span, last != 0, n, mean, div); break;
        case 32: fwht_cross_body<FORWARD, QUANT, 32>(row, col, stride, span, last != 0, n, mean, div); break;
        default: fwht_cross_body<FORWARD, QUANT, 64>(row, col, stride, span, last != 0, n, mean, div); break;
    }
