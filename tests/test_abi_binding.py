"""CPU checks of the binding that icafusion_amd/_lib.py derives from include/icaf.h: the parser on strings (what it accepts, what it refuses) and
the derived ctypes layouts against the host C compiler's view of the real header."""
import ctypes
import os
import re
import subprocess

import pytest

from helpers import REPO
from icafusion_amd import _lib
from icafusion_amd._lib import Header, IcafError, parse_header

ACCEPTED = """/* a header in the supported subset */
#ifndef DEMO_H
#define DEMO_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define ICAF_HOST
typedef void* icaf_stream_t; // hipStream_t
enum { ICAF_A = 0, ICAF_B = -3 };
typedef struct icaf_in { const void *x, *w; float alpha[2]; long long gs; } icaf_in;
typedef struct icaf_out {
    icaf_in in;          /* nested */
    const float* g[2];
    int n, reserved;
} icaf_out;
const char* icaf_name(void);
int icaf_run(ICAF_HOST const icaf_out* a, ICAF_HOST const float* const* maps, const icaf_in* dev, unsigned char* u8, double t, size_t n,
             char* buf, ICAF_HOST void** out, ICAF_HOST long long* rows, icaf_stream_t s);
#ifdef __cplusplus
}
#endif
#endif /* DEMO_H */
"""


def test_parser_reads_the_supported_subset():
    assert parse_header(ACCEPTED) == Header(
        consts={"ICAF_A": 0, "ICAF_B": -3},
        structs={"icaf_in": [("x", "void", 1, None), ("w", "void", 1, None), ("alpha", "float", 0, 2), ("gs", "long long", 0, None)],
                 "icaf_out": [("in", "icaf_in", 0, None), ("g", "float", 1, 2), ("n", "int", 0, None), ("reserved", "int", 0, None)]},
        funcs={"icaf_name": (("char", 1), []),
               "icaf_run": (("int", 0), [("a", "icaf_out", 1, True), ("maps", "float", 2, True), ("dev", "icaf_in", 1, False),
                                         ("u8", "unsigned char", 1, False), ("t", "double", 0, False), ("n", "size_t", 0, False),
                                         ("buf", "char", 1, False), ("out", "void", 2, True), ("rows", "long long", 1, True), ("s", "void", 1, False)])})


def test_binding_types_follow_the_host_mark():
    structs, sigs = _lib._bind(parse_header(ACCEPTED))
    In, Out = structs["icaf_in"], structs["icaf_out"]
    assert (In.__name__, Out.__name__) == ("In", "Out") and issubclass(Out, ctypes.Structure)
    assert [(n, getattr(In, n).offset, getattr(In, n).size) for n, _ in In._fields_] == [("x", 0, 8), ("w", 8, 8), ("alpha", 16, 8), ("gs", 24, 8)]
    assert [(n, getattr(Out, n).offset, getattr(Out, n).size) for n, _ in Out._fields_] == [("in", 0, 32), ("g", 32, 16), ("n", 48, 4), ("reserved", 52, 4)]
    assert dict(Out._fields_)["in"] is In and dict(Out._fields_)["g"] is ctypes.c_void_p * 2
    assert sigs["icaf_name"] == (ctypes.c_char_p, [])
    res, args = sigs["icaf_run"]
    assert res is ctypes.c_int
    assert args == [ctypes.POINTER(Out), ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_size_t,
                    ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_longlong), ctypes.c_void_p]


@pytest.mark.parametrize("text, quoted", [
    pytest.param("int icaf_f(unsigned short x);", "unsigned short", id="unknown-type"),
    pytest.param("int icaf_f(int (*cb)(int));", "int (*cb)(int)", id="function-pointer"),
    pytest.param("typedef struct icaf_s { int n; void (*cb)(int); } icaf_s;", "void (*cb)(int)", id="function-pointer-field"),
    pytest.param("typedef struct icaf_s { int a : 3; } icaf_s;", "int a : 3", id="bit-field"),
    pytest.param("typedef struct icaf_s { union { int a; float b; } u; } icaf_s;", "union {", id="union"),
    pytest.param("#define ICAF_N 4\nint icaf_f(void);", "#define ICAF_N 4", id="define-with-a-value"),
    pytest.param("int icaf_f(void);\nint other_f(int x);", "int other_f(int x);", id="foreign-prototype"),
    pytest.param("int icaf_f(void); static int icaf_n; int icaf_g(void);", "static int icaf_n;", id="text-left-over"),
    pytest.param("enum { ICAF_A = 1 << 2 };", "ICAF_A = 1 << 2", id="enumerator-without-a-plain-value"),
    pytest.param("int icaf_f(ICAF_HOST int x);", "ICAF_HOST int x", id="host-mark-on-a-scalar"),
    pytest.param("#ifdef DEMO\nint icaf_f(void);\n#endif", "#ifdef DEMO", id="conditional-block"),
])
def test_parser_refuses_what_it_does_not_understand(text, quoted):
    with pytest.raises(IcafError, match=re.escape(quoted)):
        parse_header(text)


def test_a_missing_header_is_reported_like_a_missing_library(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "include" / "icaf.h"))
    with pytest.raises(IcafError, match=r"icaf\.h not found"):
        _lib._load_header()


def test_derived_layouts_equal_the_compilers(tmp_path):
    """parser + ctypes against the host C compiler on the real header: sizeof of every struct, offsetof and sizeof of every field, every enum
    constant.  The program is generated from the DERIVED table, so a field the parser lost or invented does not compile or does not compare."""
    from icafusion_amd.build import hipcc
    lines, want = [], []
    for cname, cls in _lib.STRUCTS.items():
        lines.append(f'printf("S {cname} %zu\\n", sizeof({cname}));')
        want.append(f"S {cname} {ctypes.sizeof(cls)}")
        for name, _ in cls._fields_:
            lines.append(f'printf("F {cname} {name} %zu %zu\\n", offsetof({cname}, {name}), sizeof((({cname}*)0)->{name}));')
            want.append(f"F {cname} {name} {getattr(cls, name).offset} {getattr(cls, name).size}")
    for name, value in _lib.HEADER.consts.items():
        lines.append(f'printf("E {name} %d\\n", (int){name});')
        want.append(f"E {name} {getattr(_lib, name[len('ICAF_'):])}")
        assert getattr(_lib, name[len("ICAF_"):]) == value
    assert len(_lib.STRUCTS) >= 7 and len(_lib.HEADER.consts) >= 24 and len(want) >= 199        # what the header held when the test was written
    src, exe = tmp_path / "abi_layout.c", tmp_path / "abi_layout"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "icaf.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    r = subprocess.run([hipcc(), "-O0", "-x", "c", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.splitlines() == want
