"""Builds qm_door_amd/libqmgpu.so in-tree: hipcc (gfx950) for the kernels + C ABI, g++ for the host loaders.

The HIP runtime the library binds to is the one the host process already uses: under the Python harness that is the
libamdhip64 bundled with PyTorch-ROCm (two HIP/HSA runtimes in one process cannot both see the GPU); a C++ host such as
the qm_controllers plugin links the same objects against the system ROCm instead.
"""
import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
OUT = os.path.join(PKG, "libqmgpu.so")
OBJ = os.path.join(PKG, "build")
ARCH = "gfx950"


def _torch_lib_dir():
    try:
        import torch
        d = os.path.join(os.path.dirname(torch.__file__), "lib")
        if os.path.exists(os.path.join(d, "libamdhip64.so")):
            return d
    except Exception:
        pass
    return None


def _sources():
    deps = [os.path.join(PKG, "..", "include", "qmgpu.h")]
    for root, _, files in os.walk(CSRC):
        deps += [os.path.join(root, f) for f in files]
    return deps


def device_units(extra_flags=()):
    """name -> (source under csrc/, hipcc flags) of every device translation unit of the library: the one compile recipe that build_library (objects)
    and device_asm (device assembly) share."""
    extra_flags = list(extra_flags)
    # -enable-ipra=0: LLVM's interprocedural register allocation (on by default for AMDGPU) miscompiles a call on wbc_kernel's helper wavefront path in
    # some build variants of these sources (reproducer tools/wbc_variants.py --run opq); with it off every variant computes the
    # same cycle.  a variant switches it back on with extra_flags = (-mllvm, -enable-ipra=1).
    own_ipra = any(str(f).startswith("-enable-ipra") for f in extra_flags)
    base_flags = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value"]
    hip_flags = [*base_flags, *([] if own_ipra else ["-mllvm", "-enable-ipra=0"]), *extra_flags]
    # the kernel sources are written in terms of `real` (kernels/real.h) and compiled twice: fp64 = every kernel + the C ABI,
    # fp32 = the MPC kernels a second time in namespace qmk32
    # linesearch_kernel lives in a translation unit of its own, compiled with the interprocedural register allocation ON (qmgpu_ls.hip says why); a variant that sets the
    # switch itself, or the profiling build (one device symbol for all clocks), keeps the single translation unit
    timing = "-DQM_RICCATI_TIMING" in extra_flags
    split_ls = not own_ipra and not timing
    # lq_node_kernel lives in a translation unit of its own (qmgpu_lq.hip) compiled at -O2: measured 2.7 % faster than at -O3 (0.456 -> 0.443 ms, profiles/r04i_variant_timing.txt),
    # bit-identical results; the profiling build keeps the single translation unit
    split_lq = not timing
    # plant_kernel lives in a translation unit of its own (qmgpu_plant.hip says why), compiled as the rest; the profiling build keeps the single translation unit
    split_plant = not timing
    # wbc_report_kernel likewise (qmgpu_wbcreport.hip): every existing unit but `api`, which gains the entry point, is built from the sources and flags it had
    split_wbcreport = not timing
    units = {
        "api": ("qmgpu_api.hip", [*hip_flags, *(["-DQM_LS_EXTERN"] if split_ls else []), *(["-DQM_LQ_EXTERN"] if split_lq else []), *(["-DQM_PLANT_EXTERN"] if split_plant else []),
                                  *(["-DQM_WBCREPORT_EXTERN"] if split_wbcreport else [])]),
        "mpc32": ("qmgpu_mpc32.hip", [*hip_flags, "-DQM_REAL=float", "-Dqmk=qmk32"]),
    }
    if split_plant:
        units["plant"] = ("qmgpu_plant.hip", [*hip_flags, "-Dqmk=qmkplant"])
    if split_wbcreport:
        units["wbcreport"] = ("qmgpu_wbcreport.hip", [*hip_flags, "-Dqmk=qmkreport"])
    if split_ls:
        units["ls"] = ("qmgpu_ls.hip", [*base_flags, *extra_flags, "-mllvm", "-enable-ipra=1"])
    if split_lq:
        units["lq"] = ("qmgpu_lq.hip", [("-O2" if f == "-O3" else f) for f in hip_flags])
    return units


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _run_all(cmds, verbose=False, quiet=False):
    """runs independent commands in parallel; quiet: their stderr is shown only if one fails"""
    procs = []
    for c in cmds:
        if verbose:
            print(" ".join(c), file=sys.stderr)
        procs.append(subprocess.Popen(c, stderr=subprocess.PIPE if quiet else None))
    for c, pr in zip(cmds, procs):
        _, err = pr.communicate()
        if pr.returncode != 0:
            raise subprocess.CalledProcessError(pr.returncode, c, stderr=err)


def device_asm(out_dir, extra_flags=(), units=None):
    """device assembly (<out_dir>/<unit>.s) of the library's translation units -- all of them, or the names listed in `units` -- compiled exactly as
    build_library compiles them; returns the paths"""
    todo = {n: u for n, u in device_units(extra_flags).items() if units is None or n in units}
    if units is not None and set(units) - set(todo):
        raise ValueError(f"no translation unit {sorted(set(units) - set(todo))} in this build")
    os.makedirs(out_dir, exist_ok=True)
    out = [os.path.join(out_dir, n + ".s") for n in todo]
    _run_all([[_hipcc(), *flags, "--offload-device-only", "-S", os.path.join(CSRC, src), "-o", o] for (src, flags), o in zip(todo.values(), out)], quiet=True)
    return out


def build_library(force=False, verbose=False, extra_flags=(), out=None, obj_dir=None):
    OUT, OBJ = out or globals()["OUT"], obj_dir or globals()["OBJ"]
    deps = _sources() + [os.path.abspath(__file__)]
    if not force and os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps):
        return OUT
    os.makedirs(OBJ, exist_ok=True)
    units = device_units(extra_flags)
    objs = [os.path.join(OBJ, src.replace(".hip", ".o")) for src, _ in units.values()]
    host_o = os.path.join(OBJ, "host_config.o")
    cmds = [[_hipcc(), *flags, "-c", os.path.join(CSRC, src), "-o", o] for (src, flags), o in zip(units.values(), objs)]
    cmds.append(["g++", "-O2", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, "host", "host_config.cpp"), "-o", host_o])
    _run_all(cmds, verbose)
    # Inside this repository the process already holds PyTorch's bundled HIP runtime, so link against that one first; a catkin
    # workspace without PyTorch sets QMGPU_HIP_LIBDIR=/opt/rocm/lib.
    override = os.environ.get("QMGPU_HIP_LIBDIR")
    tl = None if override else _torch_lib_dir()
    libdirs = [override] if override else (([tl] if tl else []) + ["/opt/rocm/lib"])
    link = ["g++", "-shared", "-o", OUT, *objs, host_o]
    for d in libdirs:
        link += [f"-L{d}", f"-Wl,-rpath,{d}"]
    link += ["-lamdhip64", "-lstdc++", "-lm"]
    if verbose:
        print(" ".join(link), file=sys.stderr)
    subprocess.check_call(link)
    return OUT


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv, verbose=True))
