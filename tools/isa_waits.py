#!/usr/bin/env python3
"""Where do the kernels of a .hip file WAIT for memory?  A reading aid on top of tools/device_asm.py (device code only, no GPU needed):

    python tools/isa_waits.py icafusion_amd/csrc/dmff_wide.hip [more .hip files | git revisions as <rev>:<file>.hip]

Per kernel it prints
  (a) every SELF-LOOP (one basic block branching back to its own label) that holds a global / buffer load into registers (LDS-DMA loads
      are left out) AND an `s_waitcnt vmcnt(0)`: a load -> wait -> use loop pays one full memory round trip per iteration;
  (b) for every loop that holds both MFMAs and such loads, the `vmcnt` immediates of the waits that precede an MFMA inside the loop and
      their minimum: a register ring meant to keep D slices of L loads in flight should never wait below (D - 1) * L there.
It reads labels, branches, waits and opcode classes only (loops are found by layout: a branch to a label further up), and it judges
nothing: docs/HISTORY.md section 21 shows what the listing of dmff_wide.hip looked like before and after the weight ring was repaired."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import device_asm                      # noqa: E402

_LABEL = re.compile(r"^(\.L\w+):")
_VMCNT = re.compile(r"vmcnt\((\d+)\)")


def parse(lines):
    """assembly lines of one kernel -> [(label or None, opcode, operand text)]: labels and instructions in order, directives and comments dropped"""
    out = []
    for line in lines:
        t = line.split(";")[0].strip()
        if not t:
            continue
        m = _LABEL.match(t)
        if m:
            out.append((m.group(1), None, ""))
        elif not t.startswith(".") and not t.endswith(":"):
            op, _, rest = t.partition(" ")
            out.append((None, op, rest.strip()))
    return out


def is_reg_load(op, rest):
    return op.startswith(("global_load", "buffer_load", "flat_load")) and not re.search(r"\blds\b", rest)


def vmcnt_of(op, rest):
    """immediate of an s_waitcnt that names vmcnt, else None"""
    if op != "s_waitcnt":
        return None
    m = _VMCNT.search(rest)
    return int(m.group(1)) if m else None


def loops(items):
    """[(label, first index, index of the LAST branch back to it)] for every label that a branch below it names, outermost first"""
    at = {lab: i for i, (lab, _, _) in enumerate(items) if lab}
    found = {}
    for i, (_, op, rest) in enumerate(items):
        if op and op.startswith(("s_cbranch", "s_branch")):
            tgt = rest.split()[0] if rest else ""
            if tgt in at and at[tgt] < i:
                found[tgt] = (tgt, at[tgt], i)
    return sorted(found.values(), key=lambda l: (l[1], -l[2]))


def analyse(lines):
    """one kernel -> (serial, rings): serial = [{label, loads, insts}] for (a); rings = [{label, mfma, loads, waits, min, innermost}] for (b)"""
    items = parse(lines)
    ls = loops(items)
    serial, rings = [], []
    for lab, a, b in ls:
        body = items[a:b + 1]
        insts = [(op, rest) for l, op, rest in body if op]
        loads = sum(1 for op, rest in insts if is_reg_load(op, rest))
        self_loop = not any(l for l, _, _ in body[1:])
        if self_loop and loads and any(vmcnt_of(op, rest) == 0 for op, rest in insts):
            serial.append(dict(label=lab, loads=loads, insts=len(insts)))
        mf = [k for k, (op, _) in enumerate(insts) if op.startswith("v_mfma")]
        if mf and loads:
            waits = [v for v in (vmcnt_of(op, rest) for op, rest in insts[:mf[-1]]) if v is not None]
            inner = not any(a <= a2 and b2 <= b and (a2, b2) != (a, b) for _, a2, b2 in ls)
            rings.append(dict(label=lab, mfma=len(mf), loads=loads, waits=waits, min=min(waits) if waits else None, innermost=inner))
    return serial, rings


def report(kernels, pretty, out=sys.stdout):
    for name in sorted(kernels, key=lambda k: pretty.get(k, k)):
        serial, rings = analyse(kernels[name])
        print(f"{pretty.get(name, name).replace('icaf::', '')[:170]}", file=out)
        print(f"  (a) serial load loops: {len(serial)}" + "".join(f"\n      {s['label']}: {s['loads']} load(s), {s['insts']} instructions, vmcnt(0)" for s in serial),
              file=out)
        if not rings:
            print("  (b) no loop with MFMAs and loads", file=out)
        for r in rings:
            w = " ".join(map(str, r["waits"])) or "-"
            print(f"  (b) {r['label']}{' innermost' if r['innermost'] else ''}: {r['mfma']} MFMAs, {r['loads']} loads, vmcnt before an MFMA: {w}; min {r['min']}", file=out)


def main():
    from icafusion_amd import build as B
    for spec in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as td:
            path = spec
            if not os.path.exists(spec) and ":" in spec:                  # <git revision>:<file>.hip of csrc
                rev, f = spec.split(":", 1)
                path = os.path.join(td, os.path.basename(f))
                open(path, "w").write(subprocess.run(["git", "-C", ROOT, "show", f"{rev}:icafusion_amd/csrc/{os.path.basename(f)}"], check=True,
                                                     capture_output=True, text=True).stdout)
            asm = os.path.join(td, "out.s")
            flags = B.PER_FILE.get(os.path.basename(path), [])
            B.PER_FILE[os.path.basename(path)] = flags + ["-I", B.CSRC]
            try:
                device_asm.compile_asm(B, path, asm)
            finally:
                B.PER_FILE[os.path.basename(path)] = flags
            kernels = device_asm.split_kernels(open(asm).read())[0]
        print(f"== {spec}: {len(kernels)} kernels")
        report(kernels, B.demangle(sorted(kernels)))


if __name__ == "__main__":
    main()
