"""lqrrt_amd/csrc/generic_sizes.hpp on the host: the partial pairs a generic scan writes never exceed what the engine allocates.

The header is the one place generic_create (allocation) and generic_nn (launch grids) take their counts from; a few-line shim
over it is compiled with the host compiler and swept over capacities, max_wave, both table kinds and the node counts at which
the formulas change.  The same sweep is fed the formulas the engine had before the header existed (restated below as plain
arithmetic): it must flag them, which shows that the sweep catches the out-of-bounds write of a full wide table built with a
small max_wave."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = """
#include "generic_sizes.hpp"
extern "C" long long gs_written(long long N, long long W, int wide) { return (long long)lq::generic_pairs_written((size_t)N, (size_t)W, wide != 0); }
extern "C" long long gs_allocated(long long cap, long long max_wave, int wide) { return (long long)lq::generic_pairs_allocated((size_t)cap, (size_t)max_wave, wide != 0); }
extern "C" long long gs_blocks(long long count, int wide) { return (long long)lq::generic_scan_blocks((size_t)count, wide != 0); }
"""

CAPS = list(range(64, 8192 + 1, 64)) + [2 ** 18, 2 ** 18 + 64, 2 ** 20, 2 ** 20 + 64, 2 ** 22]
MAX_WAVES = (1, 2, 3, 4, 64, 4096)


@pytest.fixture(scope="module")
def gs():
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "t.cpp"), "w") as f:
        f.write(SRC)
    so = os.path.join(d, "t.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I",
                           os.path.join(ROOT, "lqrrt_amd", "csrc"), os.path.join(d, "t.cpp"), "-o", so])
    lib = C.CDLL(so)
    for f in (lib.gs_written, lib.gs_allocated, lib.gs_blocks):
        f.restype = C.c_longlong
    lib.gs_written.argtypes = [C.c_longlong, C.c_longlong, C.c_int]
    lib.gs_allocated.argtypes = [C.c_longlong, C.c_longlong, C.c_int]
    lib.gs_blocks.argtypes = [C.c_longlong, C.c_int]
    return lib


def sweep(written, allocated):
    """Every (cap, max_wave, wide, W, N) of the grid with written > allocated."""
    bad = []
    for cap in CAPS:
        for max_wave in MAX_WAVES:
            for wide in (0, 1):
                room = allocated(cap, max_wave, wide)
                for W in sorted({1, max_wave}):
                    for N in sorted({1, cap // 4, cap // 4 + 1, cap // 2, cap - 1, cap}):
                        if written(N, W, wide) > room:
                            bad.append((cap, max_wave, wide, W, N))
    return bad


def parent_written(N, W, wide):
    """The grids generic_nn launched before the shared header: nbw = min(ceil(N/64), 4096) wide, nb = min(ceil(N/256), 4096) x W."""
    return min((N + 63) // 64, 4096) if wide else min((N + 255) // 256, 4096) * W


def parent_allocated(cap, max_wave, wide):
    """What generic_create allocated before: generic_blocks * max_wave pairs, generic_blocks = min(ceil(cap/256), 4096)."""
    return min((cap + 255) // 256, 4096) * max_wave


def test_written_fits_allocated(gs):
    assert sweep(gs.gs_written, gs.gs_allocated) == []


def test_sweep_flags_the_previous_formulas():
    bad = sweep(parent_written, parent_allocated)
    assert bad, "the sweep does not see the overflow of a wide table with a small max_wave"
    assert all(wide == 1 and max_wave in (1, 2, 3) for _, max_wave, wide, _, _ in bad)      # the advisory's case and nothing else
    # wide, max_wave = 1, cap = 1024: 4 pairs allocated; N = cap/4 + 1 = 257 nodes write 5, a full table 16
    assert (1024, 1, 1, 1, 257) in bad and (1024, 1, 1, 1, 1024) in bad
    assert parent_written(320, 1, 1) == 5 > parent_allocated(1024, 1, 1) == 4                 # the example of the advisory
    # narrow tables were sized correctly all along
    assert not [b for b in bad if b[2] == 0]


def test_the_scan_counts_are_the_kernels_grids(gs):
    """One pair per workgroup: 256-node tiles (64 on the wide path), at most 4096 workgroups; the engine's launch grids are these numbers."""
    for count in (1, 63, 64, 65, 255, 256, 257, 16392, 65836, 262144, 262145, 1048576, 1048577, 2 ** 22):
        assert gs.gs_blocks(count, 0) == min((count + 255) // 256, 4096)
        assert gs.gs_blocks(count, 1) == min((count + 63) // 64, 4096)
    # the new sizing only ever adds room, and only for wide tables
    for cap in CAPS:
        for max_wave in MAX_WAVES:
            assert gs.gs_allocated(cap, max_wave, 0) == parent_allocated(cap, max_wave, 0)
            assert gs.gs_allocated(cap, max_wave, 1) == max(parent_allocated(cap, max_wave, 1), min((cap + 63) // 64, 4096))
