"""The hipcc command line of lqrrt_amd/csrc/engine.hip, in ONE place: __graft_entry__.build(), tools/build_user_system.py,
tools/kernel_resources.py (whose remarks and assembly the CPU tests read: the registers they report must be those of the
library that runs) and the measurement builds (tools/steer_phases_bench.py, tools/ablate_steer.py, tools/dare_phases.py) all
take it from here.

KERNARG_PRELOAD_DWORDS: gfx950's dispatcher can place the first dwords of a kernel's argument segment in scalar registers before
a wavefront starts (16 user SGPRs minus the argument-segment pointer: at most 14).  k_steer's hot header (csrc/steer.hpp) is
laid out for it; the flag applies to every kernel of the translation unit whose leading parameters are scalars or pointers, and
the compiler adds the prologue that loads the same dwords where the firmware does not preload.  -DLQRRT_NO_KERNARG_PRELOAD
(A/B builds) puts k_steer's header behind its by-value structs, where none of it is preloaded."""
import os

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNARG_PRELOAD_DWORDS = 14
ENGINE_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
                "-mllvm", "-amdgpu-kernarg-preload-count=%d" % KERNARG_PRELOAD_DWORDS]


def engine_source(root):
    return os.path.join(root, "lqrrt_amd", "csrc", "engine.hip")


def shared_library_command(root, out, extra=()):
    """hipcc ... engine.hip -o out (a complete liblqrrt_hip.so); `extra`: -D switches of a measurement or user build."""
    return [HIPCC] + ENGINE_FLAGS + ["-shared", "-I", os.path.join(root, "include")] + list(extra) + [engine_source(root), "-o", out]
