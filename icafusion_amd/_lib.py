"""ctypes binding of libicaf.so, derived from include/icaf.h: the header is the one definition of the C ABI.

Nothing of the header is repeated here.  `parse_header` reads its enums, structs and prototypes; the module then builds from them the constants
(ICAF_F32 -> F32), the C.Structure classes (icaf_conv_args -> ConvArgs) and SIGNATURES.  A new entry point is declared in icaf.h, with ICAF_HOST in
front of every pointer parameter that is host memory, and nowhere else.
The HIP library is the product: there is no CPU or PyTorch fallback.  `lib()` raises if the shared object is
missing or does not export every symbol of the header, so a GPU box that silently lost the extension fails loudly.
"""
import collections
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ICAF_LIB") or os.path.join(_HERE, "lib", "libicaf.so")   # ICAF_LIB: A/B a variant build (tools/)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "icaf.h")


class IcafError(RuntimeError):
    pass


# consts {name: int}; structs {C name: [(field, base type, pointer depth, array length or None)]};
# funcs {name: ((base type, pointer depth) of the result, [(parameter, base type, pointer depth, marked ICAF_HOST)])}
Header = collections.namedtuple("Header", "consts structs funcs")
_SCALARS = {"int": C.c_int, "long long": C.c_longlong, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
            "unsigned char": C.c_ubyte, "char": C.c_char}
_PREPROCESSOR = re.compile(r"#\s*(ifndef\s+\w+|endif|include\s*<[\w./]+>|define\s+\w+)")
_word = re.compile(r"[A-Za-z_]\w*").fullmatch


def parse_header(text):
    """The declarations of a header in icaf.h's C subset as a Header; IcafError quoting the text for anything else (never skipped, never guessed)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r'#ifdef\s+__cplusplus\s+(extern\s+"C"\s*\{|\})\s+#endif', " ", text)          # read as C
    for line in re.findall(r"^[ \t]*(#.*?)\s*$", text, re.M):
        if not _PREPROCESSOR.fullmatch(line):
            raise IcafError(f"icaf.h: unsupported preprocessor line {line!r}")
    rest = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M).strip()
    typedefs, consts, structs, funcs = {}, {}, {}, {}

    def decl(stmt, where):
        """`ICAF_HOST const float* a[2], *b` -> base type, host mark, [(name, pointer depth, array length or None)]"""
        tok = re.findall(r"\w+|\[\d+\]|\S", stmt)
        n = 0
        while n + 1 < len(tok) and _word(tok[n]) and (tok[n + 1] == "*" or _word(tok[n + 1])):
            n += 1
        base, depth0 = " ".join(w for w in tok[:n] if w not in ("const", "ICAF_HOST")), 0
        base, depth0 = typedefs.get(base, (base, 0))
        if base != "void" and base not in _SCALARS and base not in structs:
            raise IcafError(f"icaf.h: unknown type {base!r} in {where!r}")
        out = []
        for d in " ".join(tok[n:]).split(","):
            m = re.fullmatch(r"((?:\*|const\b|\s)*)([A-Za-z_]\w*)\s*(?:\[(\d+)\])?\s*", d)
            if not m:
                raise IcafError(f"icaf.h: cannot parse {where!r}")
            out.append((m[2], depth0 + m[1].count("*"), int(m[3]) if m[3] else None))
        return base, "ICAF_HOST" in tok[:n], out

    while rest:
        if m := re.match(r"enum\s*\{([^{}]*)\}\s*;", rest):
            for item in m[1].split(","):
                e = re.fullmatch(r"\s*(\w+)\s*=\s*(-?\d+)\s*", item)
                if not e:
                    raise IcafError(f"icaf.h: cannot parse the enumerator {item.strip()!r}")
                consts[e[1]] = int(e[2])
        elif m := re.match(r"typedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(\w+)\s*;", rest):
            *stmts, tail = m[1].split(";")
            if tail.strip():
                raise IcafError(f"icaf.h: cannot parse {tail.strip()!r} at the end of struct {m[2]}")
            fields = []
            for stmt in stmts:
                where = " ".join(stmt.split())
                base, host, names = decl(stmt, where)
                if host or (base == "void" and not all(depth for _, depth, _ in names)):
                    raise IcafError(f"icaf.h: cannot parse {where!r}")
                fields += [(name, base, depth, alen) for name, depth, alen in names]
            structs[m[2]] = fields
        elif m := re.match(r"typedef\s+void\s*\*\s*(\w+)\s*;", rest):
            typedefs[m[1]] = ("void", 1)
        elif m := re.match(r"([^;{}()]+)\(([^;{}()]*)\)\s*;", rest):
            where = " ".join(m[0].split())
            base, host, names = decl(m[1], where)
            (name, depth, alen), params = names[0], []
            if len(names) != 1 or alen is not None or host or not name.startswith("icaf_"):
                raise IcafError(f"icaf.h: not a prototype of an icaf_ function: {where!r}")
            for p in [] if m[2].strip() == "void" else m[2].split(","):
                pbase, phost, pn = decl(p, where)
                if pn[0][2] is not None or (pn[0][1] == 0 and (phost or pbase == "void")):
                    raise IcafError(f"icaf.h: cannot parse the parameter {p.strip()!r} of {where!r}")
                params.append((pn[0][0], pbase, pn[0][1], phost))
            funcs[name] = ((base, depth), params)
        else:
            raise IcafError(f"icaf.h: cannot parse {' '.join(re.match(r'[^;]*;?', rest)[0].split())[:200]!r}")
        rest = rest[m.end():].lstrip()
    return Header(consts, structs, funcs)


def _ctype(classes, base, depth, host=False, alen=None):
    """Scalars and structs by type; char* -> c_char_p; ICAF_HOST T* -> POINTER(T), ICAF_HOST T** / void** -> POINTER(c_void_p); other pointers c_void_p"""
    if depth == 0:
        t = None if base == "void" else _SCALARS.get(base) or classes[base]
    elif base == "char" and depth == 1:
        t = C.c_char_p
    elif host and (depth > 1 or base != "void"):
        t = C.POINTER(_ctype(classes, base, 0) if depth == 1 else C.c_void_p)
    else:
        t = C.c_void_p
    return t * alen if alen else t


def _bind(header):
    """Header -> ({C struct name: C.Structure class named in CamelCase without icaf_}, {function: (restype, argtypes)})"""
    classes = {}
    for cname, fields in header.structs.items():
        pyname = "".join(w.capitalize() for w in cname[len("icaf_"):].split("_"))
        classes[cname] = type(pyname, (C.Structure,), {"_fields_": [(name, _ctype(classes, base, depth, alen=alen)) for name, base, depth, alen in fields]})
    return classes, {name: (_ctype(classes, *ret), [_ctype(classes, base, depth, host) for _, base, depth, host in params])
                     for name, (ret, params) in header.funcs.items()}


def _load_header():
    if not os.path.exists(HEADER_PATH):
        raise IcafError(f"{HEADER_PATH} not found — icafusion_amd derives its binding of libicaf.so from it; it has no hand-written copy of the ABI")
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


HEADER = _load_header()                              # once per process
STRUCTS, SIGNATURES = _bind(HEADER)                  # SIGNATURES: symbol -> (restype, argtypes), every function of include/icaf.h
globals().update({cls.__name__: cls for cls in STRUCTS.values()})                   # ConvArgs, BneckArgs, Stem2Args, DmffArgs, TtaPass, FrameGeom, LossParams
globals().update({name[len("ICAF_"):]: value for name, value in HEADER.consts.items()})    # F32, ACT_SILU, LETTERBOX_LDS_BYTES, MISSRATE_MAX_DET, ...

_LIB = None


def lib():
    """Load libicaf.so once; raise (never fall back) when it is absent or incomplete."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise IcafError(f"{LIB_PATH} not found — build it with `python -m icafusion_amd.build` "
                            "(hipcc --offload-arch=gfx950); icafusion_amd has no CPU / PyTorch fallback")
        # torch first: its wheel carries its own HIP runtime, and a process in which libicaf.so brought the system's runtime in BEFORE torch
        # initialises the GPU ends up with two of them — the second reports "no ROCm-capable device" at its first launch
        # (`python __graft_entry__.py --smoke`: build() loads the library, smoke() then imports torch).  Loaded after torch, the
        # library shares the one runtime whose streams and allocations it is handed anyway.
        import torch  # noqa: F401
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError as e:
                raise IcafError(f"libicaf.so does not export {name}; rebuild it") from e
            fn.restype, fn.argtypes = res, args
        from .options import OPT                       # the library's probe knobs come from the one options object, not from its environment
        for name, value in OPT.lib_options().items():
            if handle.icaf_set_option(name.encode(), int(value)) != 0:
                raise IcafError(f"icaf_set_option({name}): {handle.icaf_last_error().decode()}")
        _LIB = handle
    return _LIB


def check(status, what=""):
    if status != 0:
        msg = lib().icaf_last_error()
        raise IcafError(f"{what} failed ({status}): {msg.decode() if msg else '?'}")
