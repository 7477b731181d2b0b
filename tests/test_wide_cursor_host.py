"""The weight-stream cursor of the DMFF token kernels on the host: tests/native/wide_cursor_check.cpp includes the kernels' own header
(icafusion_amd/csrc/wide_cursor.h), enumerates every geometry of the instantiation table of dmff_wide.hip and checks that the slices
consumed are the sequence the GEMM passes expect and that every slice requested — the refills past the end of the stream included — lies
inside its matrix.  Built with the host compiler and AddressSanitizer + UBSan and run as a program: an out-of-range refill is what a GPU
run cannot show without faulting."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_wide_cursor_sequence_and_bounds(tmp_path):
    cxx = host_compiler()
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "wide_cursor_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(REPO, "icafusion_amd", "csrc"), os.path.join(REPO, "tests", "native", "wide_cursor_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "wide cursor ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    # 4 builds x 2 paddings x (ln_qkv: every (npass, group, wave); proj_mlp: every (KS, slice, wave))
    assert "(496 streams)" in r.stdout, r.stdout
