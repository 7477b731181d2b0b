"""Compile a .hip file to gfx950 assembly with the library's own flags and split the text by kernel: the part that tools/isa_mix.py (instruction
classes) and tools/kernel_fingerprint.py (hashes) share.  Device code only, so no GPU is needed."""
import os
import re
import subprocess


def compile_asm(build, path, out):
    """`path` -> assembly file `out` with build.COMMON + build.PER_FILE[file name] (`build` = an icafusion_amd.build module, whose flags these are);
    returns the compiler's stderr, which carries the resource remarks build.parse_resources reads."""
    flags = [c for c in build.COMMON if c not in ("-fPIC", "-fvisibility=hidden")] + build.PER_FILE.get(os.path.basename(path), [])
    r = subprocess.run([build.hipcc()] + flags + ["-S", "--cuda-device-only", "-o", out, path], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {path}:\n{r.stderr[-6000:]}")
    return r.stderr


def split_kernels(text):
    """assembly text -> ({mangled kernel name: [its lines, label to .Lfunc_end, then its .amdhsa_kernel descriptor]}, [every other line]);
    amdhsa kernels only — a device function that was not inlined lands in the second list."""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    kernels, rest, cur = {}, [], None
    for line in text.split("\n"):
        t = line.strip()
        m = re.match(r"^(\S+):\s*(;.*)?$", line)
        if m and not line.startswith(".L"):
            cur = m.group(1) if m.group(1) in names else None
            if cur:
                kernels[cur] = []
        elif t.startswith(".amdhsa_kernel"):
            cur = t.split()[1]
        (kernels.setdefault(cur, []) if cur else rest).append(line)
        if t.startswith((".Lfunc_end", ".end_amdhsa_kernel")):     # (not the first s_endpgm: a kernel with a uniform early exit has several)
            cur = None
    return kernels, rest
