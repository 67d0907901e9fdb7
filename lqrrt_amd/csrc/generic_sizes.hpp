// LQRRT_MODEL_GENERIC: how many {eligible, overall} partial pairs a scan writes and how many an engine allocates -- the ONE place both
// generic_create (the allocation) and generic_nn (the launch grids) take them from.  Host-only, plain C++, no HIP types:
// tests/test_generic_sizes_cpu.py compiles it with the host compiler and sweeps written <= allocated.
//
// A scan launches min(ceil(N / tile), GENERIC_MAX_BLOCKS) workgroups per query (tile = 256 nodes on the compile-time-width path, 64 on the
// wide path; beyond that a workgroup strides over several tiles) and every workgroup writes one pair.  The compile-time-width path
// serves up to max_wave queries per launch; the wide path serves one (the batched device form is refused for wide tables), but its
// tile is a quarter of the other's, so its buffer is sized from its own tile: every N <= cap fits whatever max_wave is.
#pragma once

#include <cstddef>

namespace lq {

constexpr size_t GENERIC_MAX_BLOCKS = 4096;
constexpr size_t GENERIC_TILE = 256, GENERIC_TILE_WIDE = 64;

// workgroups (= partial pairs per query) of a scan over `count` nodes
inline size_t generic_scan_blocks(size_t count, bool wide) {
    const size_t tile = wide ? GENERIC_TILE_WIDE : GENERIC_TILE;
    const size_t nb = (count + tile - 1) / tile;
    return nb < GENERIC_MAX_BLOCKS ? nb : GENERIC_MAX_BLOCKS;
}

// pairs a scan of W queries over N nodes writes (a wide scan serves one query)
inline size_t generic_pairs_written(size_t N, size_t W, bool wide) { return generic_scan_blocks(N, wide) * (wide ? 1 : W); }

// pairs an engine of `cap` nodes and `max_wave` queries per call allocates
inline size_t generic_pairs_allocated(size_t cap, size_t max_wave, bool wide) {
    const size_t batched = generic_scan_blocks(cap, false) * max_wave;
    const size_t one_wide = generic_scan_blocks(cap, true);
    return wide && one_wide > batched ? one_wide : batched;
}

}  // namespace lq
