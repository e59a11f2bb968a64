"""Build the gfx950 library and CLIs in-tree with hipcc (no JIT, no cache).

Outputs (git-ignored, shipped to the GPU box with the tree):
  huffman_amd/lib/libhuffman_amd.so   C ABI of include/huffman_amd.h
  huffman_amd/bin/archive             drop-in for the reference `archive`
  huffman_amd/bin/extract             drop-in for the reference `extract`
"""
import concurrent.futures
import hashlib
import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
INCLUDE = os.path.join(ROOT, "include")
OBJ = os.path.join(PKG, "_build")
LIB = os.path.join(PKG, "lib", "libhuffman_amd.so")
BUILD_ID = os.path.join(PKG, "lib", "BUILD_ID")  # hash of the sources the library was built from
BIN = os.path.join(PKG, "bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"
MAX_BUILD_JOBS = 16


def lib_sources(src_dir):
    """The library's translation units: every hz_*.hip / hz_*.cpp of a source directory (names, sorted)."""
    return sorted(f for f in os.listdir(src_dir) if f.startswith("hz_") and f.endswith((".hip", ".cpp")))


def headers(src_dir, inc_dir):
    """Every header a unit may include: *.h of the source directory and the public header (paths, sorted)."""
    return sorted(os.path.join(src_dir, f) for f in os.listdir(src_dir) if f.endswith(".h")) + \
        [os.path.join(inc_dir, "huffman_amd.h")]


LIB_SOURCES = lib_sources(CSRC)
HEADERS = headers(CSRC, INCLUDE)
CFLAGS = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-result", f"--offload-arch={ARCH}"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd, verbose):
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError(f"build failed: {' '.join(cmd[:3])} ...")
    elif verbose and (r.stdout or r.stderr):
        sys.stderr.write(r.stdout + r.stderr)


def source_id(src_dir=CSRC, inc_dir=INCLUDE):
    """sha256 (16 hex digits) of every source and header the library is built from."""
    h = hashlib.sha256()
    for path in [os.path.join(src_dir, f) for f in lib_sources(src_dir)] + headers(src_dir, inc_dir):
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def build_jobs(units):
    """Compiler processes at once: one per unit, at most MAX_BUILD_JOBS, fewer when MAX_JOBS or
    CMAKE_BUILD_PARALLEL_LEVEL asks for fewer (never sized from the machine's CPU count)."""
    jobs = min(MAX_BUILD_JOBS, max(1, units))
    for var in ("MAX_JOBS", "CMAKE_BUILD_PARALLEL_LEVEL"):
        v = os.environ.get(var, "")
        if v.isdigit() and int(v) > 0:
            jobs = min(jobs, int(v))
    return jobs


def compile_library(src_dir, inc_dir, obj_dir, out, defines=(), force=False, verbose=False):
    """Compile every unit of src_dir (concurrently) into obj_dir and link them into the shared library `out`.
    Objects older than their source or any header are rebuilt, all of them with force."""
    os.makedirs(obj_dir, exist_ok=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    deps = headers(src_dir, inc_dir)
    flags = CFLAGS + [f"-I{inc_dir}", f"-I{src_dir}"] + list(defines)
    cmds, objs = [], []
    for src in lib_sources(src_dir):
        path = os.path.join(src_dir, src)
        obj = os.path.join(obj_dir, src + ".o")
        objs.append(obj)
        if force or _stale(obj, [path] + deps):
            lang = ["-x", "hip"] if src.endswith(".hip") else []
            cmds.append([HIPCC] + flags + lang + ["-c", path, "-o", obj])
    if cmds:
        with concurrent.futures.ThreadPoolExecutor(build_jobs(len(cmds))) as pool:
            for f in [pool.submit(_run, c, verbose) for c in cmds]:
                f.result()
    if force or _stale(out, objs):
        _run([HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", out] + objs, verbose)
    return out


def build_variant(name, defines, verbose=False):
    """An A/B build of the library with extra -D flags into huffman_amd/lib_<name>/
    (loaded with HZ_LIB_VARIANT=lib_<name>; tools/ab.sh)."""
    return compile_library(CSRC, INCLUDE, os.path.join(PKG, "_build_" + name),
                           os.path.join(PKG, "lib_" + name, "libhuffman_amd.so"), defines, True, verbose)


def build(verbose=False, force=False):
    os.makedirs(BIN, exist_ok=True)
    compile_library(CSRC, INCLUDE, OBJ, LIB, (), force, verbose)
    sid = source_id()
    if not os.path.exists(BUILD_ID) or open(BUILD_ID).read().strip() != sid:
        with open(BUILD_ID, "w") as f:
            f.write(sid + "\n")
    for name in ("archive", "extract"):
        src = os.path.join(CSRC, f"cli_{name}.cpp")
        out = os.path.join(BIN, name)
        if force or _stale(out, [src, LIB] + HEADERS):
            _run([HIPCC] + CFLAGS + [f"-I{INCLUDE}", f"-I{CSRC}", src, "-o", out, f"-L{os.path.dirname(LIB)}",
                                     "-lhuffman_amd", "-Wl,-rpath,$ORIGIN/../lib"], verbose)
    return LIB


if __name__ == "__main__":
    if "--variant" in sys.argv:  # python huffman_amd/build.py --variant NAME -DFLAG ...
        i = sys.argv.index("--variant")
        print(build_variant(sys.argv[i + 1], [a for a in sys.argv[i + 2:] if a.startswith("-D")], "-v" in sys.argv))
    else:
        build(verbose="-v" in sys.argv, force="-f" in sys.argv)
        print(LIB)
