"""CPU-side pins of k_steer's entry: the hot argument header is preloaded by the dispatcher in every instantiation, it costs no
scratch, no occupancy and no registers, and the round block's layout is the same function on the host and in the device pass
and keeps its arrays apart.  hipcc cross-compiles for gfx950 here; the library's own assembly and remarks come from the cache
that the build fills (tools/kernel_resources.py), the two small translation units below compile in seconds."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import engine_flags
import kernel_resources as kr

USER = ["-DLQRRT_USER_SYSTEM=\"%s\"" % os.path.join(ROOT, "examples", "user_system", "unicycle.hpp")]
SIZES = (1, 63, 64, 65, 256, 1024)
FIELDS = ("ctl", "M0", "M1", "lf0", "lf1", "par0", "par1", "stale0", "stale1", "changed0", "changed1", "bytes")


def _need_hipcc():
    if not shutil.which(kr.HIPCC) and not os.path.exists(kr.HIPCC):
        pytest.skip("hipcc not available")


def _hot_dwords():
    text = open(os.path.join(ROOT, "lqrrt_amd", "csrc", "steer.hpp")).read()
    return int(re.search(r"STEER_HOT_DWORDS = (\d+)", text).group(1))


def _device_compile(body, extra=()):
    """Assembly and resource remarks of a small translation unit that includes kernels.hpp, built with the engine's flags."""
    d = tempfile.mkdtemp()
    src, asm = os.path.join(d, "tu.hip"), os.path.join(d, "tu.s")
    with open(src, "w") as f:
        f.write('#include <hip/hip_runtime.h>\n#include "kernels.hpp"\nnamespace lq {\n%s\n}\n' % body)
    done = subprocess.run([kr.HIPCC] + engine_flags.ENGINE_FLAGS + ["-S", "--cuda-device-only", kr.REMARK_FLAG, "-I",
                           os.path.join(ROOT, "lqrrt_amd", "csrc"), "-I", os.path.join(ROOT, "include"), src, "-o", asm] + list(extra),
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    return open(asm).read(), done.stderr


def _descriptors(text, prefix):
    """{kernel symbol: its .amdhsa_kernel block} for the symbols that begin with `prefix`."""
    return {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S)
            if m.group(1).startswith(prefix)}


def test_header_width_is_the_build_flag():
    assert _hot_dwords() == engine_flags.KERNARG_PRELOAD_DWORDS <= 14          # 16 user SGPRs minus the argument-segment pointer
    assert "-amdgpu-kernarg-preload-count=%d" % _hot_dwords() in engine_flags.ENGINE_FLAGS


def test_every_steer_instantiation_preloads_the_hot_header_and_uses_no_scratch():
    _need_hipcc()
    desc = _descriptors(kr.device_asm(USER), "_ZN2lq7k_steerI")
    assert len(desc) >= 14 and any("UserSystem" in k for k in desc)
    for name, block in desc.items():
        m = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", block)
        assert m and int(m.group(1)) == _hot_dwords(), (name, m and m.group(1))
        assert re.search(r"\.amdhsa_user_sgpr_kernarg_preload_offset 0\b", block), name
    # scratch: the rule of tests/test_abi_cpu.py test_steer_kernels_use_no_scratch, on the remarks of the same compile
    steer = [r for r in kr.parse(kr.remarks(USER)) if "k_steer<" in r["name"]]
    assert len(steer) == len(desc)
    framed = [r for r in steer if r["scratch"] != 0]
    assert all(r["scratch"] <= 64 for r in framed), [(r["name"][:60], r["scratch"]) for r in framed]
    if framed:
        touched = kr.private_memory_instructions([r["mangled"] for r in framed], USER)
        assert all(v == 0 for v in touched.values()), touched


HOT = "double*, const double*, const Part*, unsigned char*, int, int, int, int, int, int"
ONE_STEER = ("#ifndef LQRRT_NO_KERNARG_PRELOAD\n"
             "template __global__ void k_steer<BoatAdvanced, 0, 3>(%s, SteerCold);\n"
             "#else\n"
             "template __global__ void k_steer<BoatAdvanced, 0, 3>(Params, Geo, Res, TreeView, RecLayout, const int*, const int*, const int*, "
             "SteerFuse, RoundArgs, %s);\n"
             "#endif\n" % (HOT, HOT))


def test_the_header_costs_the_chain_rollout_no_occupancy_and_no_registers():
    """k_steer<BoatAdvanced, 0, 3>, the bench's kernel, against the same source built with the header behind the structs."""
    _need_hipcc()
    rows = {}
    for tag, extra in (("preload", []), ("no_preload", ["-DLQRRT_NO_KERNARG_PRELOAD"])):
        text, remarks = _device_compile(ONE_STEER, extra)
        r = [r for r in kr.parse(remarks) if "k_steer<" in r["name"]]
        assert len(r) == 1
        rows[tag] = r[0]
        d = _descriptors(text, "_ZN2lq7k_steerI")
        assert len(d) == 1
        want = _hot_dwords() if tag == "preload" else 0
        m = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", list(d.values())[0])
        assert (int(m.group(1)) if m else 0) == want, (tag, m and m.group(1))
    print("k_steer<BoatAdvanced, 0, 3>:", {k: (v["vgpr"], v["sgpr"], v["scratch"], v["occupancy"]) for k, v in rows.items()})
    assert rows["preload"]["occupancy"] >= rows["no_preload"]["occupancy"]
    assert rows["preload"]["vgpr"] <= rows["no_preload"]["vgpr"]
    assert rows["preload"]["scratch"] == 0


def _host_layout(maxW):
    from lqrrt_amd import _native as nat
    out = (C.c_longlong * 12)()
    fn = nat.lib().lqrrt_debug_round_layout
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.POINTER(C.c_longlong)]
    assert fn(maxW, out) == 0
    return dict(zip(FIELDS, list(out)))


def _device_layouts():
    """round_layout() as the DEVICE pass of the compiler evaluates it: a constant table in the device assembly."""
    row = ("{round_layout(%d).ctl, round_layout(%d).M[0], round_layout(%d).M[1], round_layout(%d).lf[0], round_layout(%d).lf[1], "
           "round_layout(%d).par[0], round_layout(%d).par[1], round_layout(%d).stale[0], round_layout(%d).stale[1], "
           "round_layout(%d).changed[0], round_layout(%d).changed[1], round_layout(%d).bytes}")
    body = ('extern "C" __device__ __attribute__((used)) const long long round_layout_device_table[%d][12] = {%s};'
            % (len(SIZES), ", ".join(row % ((w,) * 12) for w in SIZES)))
    text, _ = _device_compile(body)
    m = re.search(r"\nround_layout_device_table:\n(.*?)\n\s*\.size\s+round_layout_device_table", text, re.S)
    assert m, "table not found in the device assembly"
    vals = []
    for ln in m.group(1).splitlines():
        q = re.match(r"\s*\.quad\s+(-?\d+)", ln)
        z = re.match(r"\s*\.zero\s+(\d+)", ln)
        if q:
            vals.append(int(q.group(1)))
        elif z:
            vals += [0] * (int(z.group(1)) // 8)
    assert len(vals) == 12 * len(SIZES), len(vals)
    return {w: dict(zip(FIELDS, vals[12 * i:12 * i + 12])) for i, w in enumerate(SIZES)}


def test_round_block_layout_host_equals_device_and_keeps_its_arrays_apart():
    _need_hipcc()
    dev = _device_layouts()
    for w in SIZES:
        L = _host_layout(w)
        assert L == dev[w], (w, L, dev[w])
        # sizes in bytes: control block of 16 ints, two 256 x 256 matrices of doubles, {len, flags} ints, parent ints, two byte arrays
        size = dict(ctl=64, M0=8 * 256 * 256, M1=8 * 256 * 256, lf0=8 * w, lf1=8 * w, par0=4 * w, par1=4 * w,
                    stale0=w, stale1=w, changed0=w, changed1=w)
        spans = sorted((L[k], L[k] + size[k], k) for k in size)
        assert spans[0][0] == 0
        for (a0, a1, ka), (b0, b1, kb) in zip(spans, spans[1:]):
            assert a1 <= b0, (w, ka, kb)
        assert spans[-1][1] <= L["bytes"]
        for k in ("ctl", "M0", "M1", "lf0", "lf1"):                 # doubles and the 64-bit round words (two ints per sample too)
            assert L[k] % 8 == 0, (w, k)
        for k in ("par0", "par1"):
            assert L[k] % 4 == 0, (w, k)
