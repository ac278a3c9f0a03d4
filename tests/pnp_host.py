"""TEST INFRASTRUCTURE. The host build of ground-fusion2_amd/csrc/gfbe_pnp.h with a plain C++ compiler (g++ -O2 -ffp-contract=off, no HIP):
tests/pnp_host_shim.cpp as a shared library behind ctypes, for tests/test_pnp_model.py and tools/diag_pnp_bench.py, and the compile step
the sanitized stand-alone program shares."""
import ctypes as C
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
HEADER = os.path.join(ROOT, "ground-fusion2_amd", "csrc", "gfbe_pnp.h")
PF, PI, PD, PU8 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)


def build(src, out, extra):
    """src -> out when out is older than src or the header; returns out"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    if not cxx:
        raise RuntimeError("no C++ compiler: gfbe_pnp.h cannot be built for the host")
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in (src, HEADER)):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off"] + extra + ["-o", out, src], check=True)
    return out


def load_shim():
    lib = C.CDLL(build(os.path.join(ROOT, "tests", "pnp_host_shim.cpp"), os.path.join(BUILD, "pnp_host_shim.so"), ["-fPIC", "-shared"]))
    lib.shim_pnp_hash.restype, lib.shim_pnp_hash.argtypes = C.c_uint64, [C.c_uint64, C.c_int, C.c_int]
    lib.shim_pnp_sample.argtypes = [C.c_uint64, C.c_int, C.c_int, PI]
    lib.shim_pnp_p3p.argtypes = [PD, PD, PD]
    lib.shim_pnp_solve6.argtypes = [PD, PD]
    lib.shim_pnp_rot_to_quat.argtypes = [PD, PD]
    lib.shim_pnp_normalize_angle.restype, lib.shim_pnp_normalize_angle.argtypes = C.c_double, [C.c_double]
    lib.shim_pnp_verify.argtypes = [C.c_int, PI, PF, PF, PD, PD, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_double, C.c_double, C.c_double, PU8, PI, PI, PD, PD, PI, PI, PI, PI, PD,
                                    PI]
    return lib
