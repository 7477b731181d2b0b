"""tools/kernel_fingerprint.py: the device-code fingerprint is blind to source text that compiles to nothing and sees one live constant.  Compiles
three ten-line kernels for gfx950 (device code only: no GPU needed)."""
import importlib.util
import os
import subprocess
import sys

import pytest

from helpers import REPO
from icafusion_amd import build

TOOL = os.path.join(REPO, "tools", "kernel_fingerprint.py")
KERNEL = """#include <hip/hip_runtime.h>
// %(comment)s
extern "C" __global__ void scale_kernel(float* x, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v = x[i] * %(factor)s;
    if constexpr (false) { %(dead)s }
    x[i] = v;
}
"""


def _hipcc_present():
    try:
        return subprocess.run([build.hipcc(), "--version"], capture_output=True).returncode == 0
    except (OSError, RuntimeError):
        return False


@pytest.mark.skipif(not _hipcc_present(), reason="hipcc is not installed: nothing can be compiled to gfx950 assembly here")
def test_fingerprint_ignores_dead_code_and_sees_a_live_constant(tmp_path):
    spec = importlib.util.spec_from_file_location("kernel_fingerprint", TOOL)
    kf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kf)
    variants = {"a": dict(comment="first wording", factor="3.0f", dead=""),
                "b": dict(comment="second wording, longer than the first", factor="3.0f", dead="v = v * 5.0f + 1.0f;"),
                "c": dict(comment="first wording", factor="3.5f", dead="")}
    for name, v in variants.items():
        (tmp_path / name).mkdir()
        (tmp_path / name / "k.hip").write_text(KERNEL % v)
    fa, fb = kf.fingerprint(str(tmp_path / "a")), kf.fingerprint(str(tmp_path / "b"))
    key = ("k.hip", "scale_kernel")
    assert set(fa) == {key, ("k.hip", "(rest)")}
    assert fa == fb                                                   # hashes AND resources, kernel and rest of the file
    assert {"vgpr", "sgpr", "lds", "scratch"} <= set(fa[key][1]) and fa[key][1]["scratch"] == 0

    saved = tmp_path / "a.fp"
    saved.write_text("".join(kf.line(k, fa[k]) + "\n" for k in sorted(fa)))
    assert kf.fingerprint(str(saved)) == fa                           # the printed form reads back
    same = subprocess.run([sys.executable, TOOL, "--diff", str(saved), str(tmp_path / "b")], capture_output=True, text=True)
    assert same.returncode == 0 and "1 kernels in 1 files compared: 0 differ" in same.stdout, same.stdout + same.stderr
    diff = subprocess.run([sys.executable, TOOL, "--diff", str(saved), str(tmp_path / "c")], capture_output=True, text=True)
    assert diff.returncode != 0, diff.stdout + diff.stderr
    assert any(l.startswith("differs") and l.endswith(" scale_kernel") for l in diff.stdout.splitlines()), diff.stdout
    assert "1 differ" in diff.stdout.splitlines()[-1]
