// The body of k_planar_emit and k_planar_emit_l (planar.hip), included into both so that the kernel of every block stays the code
// that was timed.  From the kernel: planar, g, nblocks, dst, choice, n and the constant kLadder -- false: every element (choice and n
// are not looked at); true: the elements of a block whose choice lies outside the ladder of n entries are passed over (the
// inverse transform has left the block alone, k_fwht_l).  A thread's elements ascend, so the block of an element is looked up
// only where it leaves the last one's.
    const uint32_t sx = 32u - 8u * g.bps;
    const uint64_t total = (uint64_t)nblocks * g.N;
    [[maybe_unused]] uint64_t lim = 0;  // the first element behind the block that `skip` was read for
    [[maybe_unused]] bool skip = false;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256u) {
        if (kLadder) {
            if (i >= lim) {
                const uint64_t b = i / g.N;
                lim = (b + 1) * g.N;
                skip = choice[b] >= n;
            }
            if (skip) continue;
        }
        dst[i] = (int32_t)cut_to_width((uint32_t)planar[i], sx);
    }
