#!/usr/bin/env python3
"""Fingerprint of the device code a source tree compiles to: the counterpart of tools/plan_fingerprint.py for the kernels.

    python tools/kernel_fingerprint.py [TREE | --ref COMMIT]
    python tools/kernel_fingerprint.py --diff A B

Compiles every .hip file of a tree to gfx950 assembly with the library's own flags (build.COMMON + build.PER_FILE of THAT tree, device code only, no
GPU needed) and prints one line per kernel: file, sha256 of the kernel's assembly text (body and kernel descriptor), its registers / LDS / scratch
from the resource remarks, and the demangled name.  One more line per file, `(rest)`, hashes everything outside the kernels (constant tables, device
functions that were not inlined, metadata).  Lines that carry the per-translation-unit `__hip_cuid_...` symbol are dropped: it is a hash of the source
text and differs between any two sources.  The tool compares text; it looks at no instruction.

A tree is a directory — a checkout (its icafusion_amd/csrc is compiled) or a bare directory of .hip files (compiled with this checkout's flags) — or,
for --ref and --diff, a file that holds this tool's output (nothing is compiled) or anything else `git archive` accepts as a commit of this
repository.  --diff prints the kernels that differ, appeared or vanished between two trees and exits non-zero if any did: a refactor that must
not touch the device code ends with "0 differ" over every instantiation, launched by a test or not."""
import argparse
import concurrent.futures as cf
import hashlib
import importlib.util
import io
import os
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import device_asm                      # noqa: E402

JOBS = min(16, os.cpu_count() or 1)
SHOWN = ("vgpr", "agpr", "sgpr", "lds", "scratch")     # resources printed next to the hash (and compared with it)


def build_module(tree):
    """icafusion_amd/build.py of `tree` (flags only: it is loaded by path, the package around it is not imported); this checkout's for a bare directory"""
    path = os.path.join(tree, "icafusion_amd", "build.py")
    if not os.path.exists(path):
        path = os.path.join(ROOT, "icafusion_amd", "build.py")
    spec = importlib.util.spec_from_file_location("icaf_build_" + hashlib.sha256(path.encode()).hexdigest()[:12], path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def fingerprint(tree):
    """{(file, demangled kernel name or "(rest)"): (sha256, resources)} of a directory, or read back from a file of printed lines"""
    if os.path.isfile(tree):
        with open(tree) as f:
            return dict(parse(l) for l in f.read().splitlines() if l)
    build = build_module(tree)
    csrc = os.path.join(tree, "icafusion_amd", "csrc")
    csrc = csrc if os.path.isdir(csrc) else tree
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))

    def one(src):
        out = os.path.join(td, src[:-4] + ".s")
        res = build.parse_resources(device_asm.compile_asm(build, os.path.join(csrc, src), out))
        with open(out) as f:
            kernels, rest = device_asm.split_kernels(f.read())
        return src, kernels, rest, res

    def digest(lines):
        return hashlib.sha256("\n".join(l for l in lines if "__hip_cuid_" not in l).encode()).hexdigest()[:16]

    fp = {}
    with tempfile.TemporaryDirectory() as td, cf.ThreadPoolExecutor(JOBS) as ex:
        for src, kernels, rest, res in ex.map(one, srcs):
            pretty = build.demangle(sorted(kernels))
            for k, lines in kernels.items():
                fp[(src, pretty[k])] = (digest(lines), {r: v for r, v in res.get(k, {}).items() if r in SHOWN})
            fp[(src, "(rest)")] = (digest(rest), {})
    return fp


def resolve(stack, tree):
    """a directory or file as it is; a commit exported into a temporary directory that lives as long as `stack`"""
    if os.path.exists(tree):
        return os.path.abspath(tree)
    td = stack.enter_context(tempfile.TemporaryDirectory())
    tar = subprocess.run(["git", "-C", ROOT, "archive", tree, "icafusion_amd/build.py", "icafusion_amd/csrc", "include"], check=True, capture_output=True).stdout
    tarfile.open(fileobj=io.BytesIO(tar)).extractall(td)
    return td


def line(key, val):
    (src, name), (h, r) = key, val
    res = " ".join(f"{k}={r[k]}" for k in SHOWN if k in r)
    return f"{src} {h} [{res}] {name}"


def parse(text):
    src, h, tail = text.split(" ", 2)
    res, name = tail[1:].split("] ", 1)
    return (src, name), (h, {k: int(v) for k, v in (kv.split("=") for kv in res.split())})


def main():
    import contextlib
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("tree", nargs="?", default=ROOT, help="directory to fingerprint (default: this checkout)")
    ap.add_argument("--ref", help="fingerprint this commit instead")
    ap.add_argument("--diff", nargs=2, metavar=("A", "B"), help="compare two trees (directories or commits)")
    a = ap.parse_args()
    with contextlib.ExitStack() as stack:
        if not a.diff:
            fp = fingerprint(resolve(stack, a.ref or a.tree))
            for k in sorted(fp):
                print(line(k, fp[k]))
            print(f"{sum(n != '(rest)' for _, n in fp)} kernels in {len({s for s, _ in fp})} files", file=sys.stderr)
            return 0
        fa, fb = (fingerprint(resolve(stack, t)) for t in a.diff)
    changed = 0
    for k in sorted(set(fa) | set(fb)):
        if k not in fb:
            print("vanished  " + line(k, fa[k]))
        elif k not in fa:
            print("appeared  " + line(k, fb[k]))
        elif fa[k] != fb[k]:
            print("differs   " + line(k, fa[k]) + "\n       ->  " + line(k, fb[k]))
        else:
            continue
        changed += 1
    nk = sum(n != "(rest)" for _, n in set(fa) | set(fb))
    print(f"{nk} kernels in {len({s for s, _ in set(fa) | set(fb)})} files compared: {changed} differ, appeared or vanished")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
