"""In-tree builds of the native pieces (no network, no cmake needed).

  libsdfgpu.so   HIP kernels + C ABI (include/sdfgpu.h): every csrc/*.hip, hipcc --offload-arch=gfx950
  pysdf_tools    pybind11 module mirroring the reference's src/sdf_tools/bindings.cpp

hipcc cross-compiles gfx950 without a GPU, so this runs in the CPU container;
the built .so files travel to the GPU box with the repo snapshot.
"""
import os
import subprocess
import sys
import sysconfig

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
INCLUDE = os.path.join(ROOT, "include")
LIB = os.path.join(PKG, "libsdfgpu.so")
LIB_MULTI = os.path.join(PKG, "libsdfgpu_multi.so")


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _hipcc():
    for c in ("/opt/rocm/bin/hipcc", "hipcc"):
        if os.path.exists(c) or c == "hipcc":
            return c


def _depfile_sources(depfile):
    """The files a Makefile-style depfile (hipcc -MD -MF) names as prerequisites; None when it is missing or unreadable.
    Split on whitespace: a path with a space in it (written as `\\ `) comes out as names that do not exist, which _stale reads as
    "rebuild" -- such a tree over-builds on every run and never goes stale."""
    try:
        text = open(depfile).read()
    except OSError:
        return None
    words = text.replace("\\\n", " ").split()
    return [w for w in words if not w.endswith(":")]


def _stale(obj, src):
    """An object is rebuilt when it or its depfile is missing, or when its source or any file the depfile names is newer."""
    deps = _depfile_sources(obj + ".d")
    if deps is None or not os.path.exists(obj):
        return True
    t = os.path.getmtime(obj)
    return any(not os.path.exists(d) or os.path.getmtime(d) > t for d in [src] + deps)


def build_libsdfgpu(force=False, verbose=False):
    """Every csrc/*.hip -> an object (compiled side by side) -> libsdfgpu.so.  DESIGN.md section 5 has the table of the units:
    sdfgpu.hip (the SDF build: its C ABI, host orchestration and most kernels), sdfgpu_context.hip (the handle), the two
    instantiation units (sdfgpu_envelope_tu.hip, sdfgpu_dense6_tu.hip) and one unit per family with its kernels, launchers, host
    code and entry points (components, topology, surfaces, convex, project, query, batch, resample, display, scene, mesh;
    mesh_solid holds the solid fill's kernels and the closedness check, its entry points sit in mesh).

    Dependencies are the compiler's: each compile writes <obj>.d (-MD -MF), and an object is rebuilt when its source or ANY file
    named there is newer, or when the depfile is missing (a stale library after a header-only edit is the kind of bug that
    invalidates measurements without failing anything)."""
    from concurrent.futures import ThreadPoolExecutor
    units = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))
    objdir = os.path.join(CSRC, ".obj")
    os.makedirs(objdir, exist_ok=True)
    todo, objs = [], []
    for src in units:
        obj = os.path.join(objdir, os.path.basename(src)[:-4] + ".o")
        objs.append(obj)
        if force or _stale(obj, src):
            todo.append([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-pthread", "-I", INCLUDE, "-MD", "-MF", obj + ".d",
                         "-c", src, "-o", obj])
    if not todo and not _newer(LIB, objs):
        return LIB
    if verbose:
        for cmd in todo:
            print(" ".join(cmd))
    with ThreadPoolExecutor(max_workers=8) as pool:
        list(pool.map(subprocess.check_call, todo))
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"] + objs + ["-o", LIB]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB


def build_libsdfgpu_multi(force=False, verbose=False):
    """libsdfgpu_multi.so: the multi-GPU C ABI (include/sdfgpu_multi.h) over libsdfgpu.so + RCCL.  Host code only."""
    src = os.path.join(CSRC, "sdfgpu_multi.cpp")
    deps = [src, os.path.join(INCLUDE, "sdfgpu_multi.h"), os.path.join(INCLUDE, "sdfgpu.h")]
    build_libsdfgpu(force=False, verbose=verbose)
    if not force and not _newer(LIB_MULTI, deps + [LIB]):
        return LIB_MULTI
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I", INCLUDE, "-I", "/opt/rocm/include",
           src, "-o", LIB_MULTI, "-L", PKG, "-lsdfgpu", "-L", "/opt/rocm/lib", "-lrccl", "-Wl,-rpath,$ORIGIN",
           "-Wl,-rpath,/opt/rocm/lib"]          # (librccl.so is found without LD_LIBRARY_PATH: pysdf_tools links this library)
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB_MULTI


def pysdf_tools_path():
    suffix = sysconfig.get_config_var("EXT_SUFFIX") or ".so"
    return os.path.join(PKG, "pysdf_tools" + suffix)


def build_pysdf_tools(force=False, verbose=False):
    import pybind11

    src = os.path.join(CSRC, "pysdf_tools.cpp")
    if not os.path.exists(src):
        return None
    out = pysdf_tools_path()
    hdr_dir = os.path.join(INCLUDE, "sdf_tools")
    deps = [src, os.path.join(INCLUDE, "sdfgpu.h"), os.path.join(INCLUDE, "sdfgpu_multi.h")] + \
        [os.path.join(hdr_dir, f) for f in sorted(os.listdir(hdr_dir))] + \
        [os.path.join(INCLUDE, "arc_utilities", f) for f in sorted(os.listdir(os.path.join(INCLUDE, "arc_utilities")))]
    if not force and not _newer(out, deps):
        return out
    build_libsdfgpu_multi(force=False, verbose=verbose)
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-DSDF_TOOLS_MULTI_GPU", "-DSDF_TOOLS_VECTOR_ADOPT",
           "-I", INCLUDE, "-I", pybind11.get_include(), "-I", sysconfig.get_paths()["include"],
           src, "-o", out, "-L", PKG, "-lsdfgpu_multi", "-lsdfgpu", "-Wl,-rpath,$ORIGIN", "-lz"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


def build_example(name, force=False, verbose=False):
    """examples/<name>.cpp -> examples/<name>_example with g++ against include/ and the in-tree libsdfgpu.so (the C++ side of
    the drop-in boundary: client code written like the reference's, tests/test_cpp_example.py and bench.py run these)."""
    src = os.path.join(ROOT, "examples", name + ".cpp")
    exe = os.path.join(ROOT, "examples", name + "_example")
    hdr_dir = os.path.join(INCLUDE, "sdf_tools")
    deps = [src, os.path.join(INCLUDE, "sdfgpu.h")] + [os.path.join(hdr_dir, f) for f in sorted(os.listdir(hdr_dir))] + \
        [os.path.join(INCLUDE, "arc_utilities", f) for f in sorted(os.listdir(os.path.join(INCLUDE, "arc_utilities")))]
    build_libsdfgpu(force=False, verbose=verbose)
    if not force and not _newer(exe, deps):
        return exe
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-DSDF_TOOLS_VECTOR_ADOPT", "-I", INCLUDE, src, "-o", exe, "-L", PKG, "-lsdfgpu",
           "-Wl,-rpath," + PKG, "-lz"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return exe


def build_all(force=False, verbose=False):
    out = [build_libsdfgpu(force, verbose), build_libsdfgpu_multi(force, verbose)]
    p = build_pysdf_tools(force, verbose)
    if p:
        out.append(p)
    out.append(build_example("class_seam", force, verbose))     # (bench.py's host_api.class_seam runs it on the GPU box)
    return out


if __name__ == "__main__":
    print("\n".join(build_all(force="--force" in sys.argv, verbose=True)))
