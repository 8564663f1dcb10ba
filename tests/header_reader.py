"""Reader of include/unimm_hip.h for tests/test_abi.py: its prototypes, argument structs and constants as plain data, and the
comparisons of each with the binding's tables (`lib.SIGNATURES`, `lib.STRUCTS`).  It reads this header's style with regular
expressions, it is no C parser; a declaration it cannot read raises instead of being skipped."""
import ctypes as C
import re

SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "float": C.c_float,
           "double": C.c_double}


def ctype(ctext, result=False):
    """The ctypes type of a C type: any pointer is c_void_p (a `const char*` RESULT is c_char_p), scalars by SCALARS."""
    t = " ".join(ctext.replace("*", " * ").split())
    if "*" in t:
        return C.c_char_p if result and t == "const char *" else C.c_void_p
    t = t[len("const "):] if t.startswith("const ") else t
    if t not in SCALARS:
        raise ValueError(f"type {ctext!r} is not in the mapping")
    return SCALARS[t]


def _code(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def constants(text):
    """{name: value} of every `#define NAME integer` (the include guard has no value) and every enum constant."""
    code, out = _code(text), {}
    for line in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(.*)$", code, flags=re.M):
        m = re.fullmatch(r"(\w+)(?:\s+\(?\s*(-?\d+)\s*\)?)?", line.strip())
        if m is None or (m.group(2) is None and not m.group(1).endswith("_H")):
            raise ValueError(f"cannot read '#define {line}'")
        if m.group(2) is not None:
            out[m.group(1)] = int(m.group(2))
    for body in re.findall(r"\benum\s*\{([^}]*)\}", code):
        value = 0
        for item in filter(None, (i.strip() for i in body.split(","))):
            m = re.fullmatch(r"(\w+)(?:\s*=\s*(-?\d+))?", item)
            if m is None:
                raise ValueError(f"cannot read enum item {item!r}")
            value = int(m.group(2)) if m.group(2) is not None else value
            out[m.group(1)] = value
            value += 1
    return out


_STRUCT = r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;"


def structs(text):
    """{struct name: [(field, ctypes type, array length or None), ...]} of every `typedef struct { ... } name;`, in order."""
    consts, out = constants(text), {}
    for body, name in re.findall(_STRUCT, _code(text)):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.fullmatch(r"((?:const\s+)?\w+)\b\s*(.*)", decl, flags=re.S)          # `const float` + `* a, * b[4]`
            if m is None:
                raise ValueError(f"{name}: cannot read {decl!r}")
            for declarator in m.group(2).split(","):
                d = re.fullmatch(r"(\**)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?", declarator.strip())
                if d is None:
                    raise ValueError(f"{name}: cannot read {decl!r}")
                n = d.group(3)
                length = None if n is None else int(n) if n.isdigit() else consts[n]
                fields.append((d.group(2), ctype(m.group(1) + d.group(1)), length))
        out[name] = fields
    return out


def _prototypes(text):
    code = re.sub(_STRUCT, " ", _code(text))
    code = re.sub(r"\benum\s*\{[^}]*\}\s*;", " ", code)
    code = re.sub(r"^[ \t]*#.*$", " ", code, flags=re.M).replace('extern "C" {', " ")
    *statements, tail = code.split(";")
    if tail.strip() != "}":                                  # the closing brace of extern "C"
        raise ValueError(f"cannot read the end of the header: {tail.strip()!r}")
    for st in statements:
        m = re.fullmatch(r"(.*?)\b(\w+)\s*\((.*)\)", st.strip(), flags=re.S)
        if m is None:
            raise ValueError(f"cannot read {st.strip()!r}")
        args = []
        if m.group(3).strip() != "void":
            for a in m.group(3).split(","):
                am = re.fullmatch(r"(.*[\s*])(\w+)", a.strip(), flags=re.S)
                if am is None:
                    raise ValueError(f"{m.group(2)}: cannot read parameter {a.strip()!r}")
                args.append((ctype(am.group(1)), am.group(2), " ".join(am.group(1).split())))
        yield m.group(2), ctype(m.group(1), result=True), args


def prototypes(text):
    """[(name, result ctypes type, [argument ctypes types]), ...] of every function the header declares, in order."""
    return [(name, res, [a[0] for a in args]) for name, res, args in _prototypes(text)]


def streamed(text):
    """names of the prototypes whose last parameter is `void* stream`"""
    return {name for name, _, args in _prototypes(text) if args and args[-1][1:] == ("stream", "void*")}


def pointer_params(text):
    """{prototype name: [(argument index, parameter name, C type text, is const, pointee struct name or None)]} of every pointer
    parameter: what tests/stream_trace.py checks the raw arguments of each call against."""
    names = set(structs(text))
    out = {}
    for name, _, args in _prototypes(text):
        rows = []
        for i, (_, pname, ctext) in enumerate(args):
            if "*" in ctext:
                base = ctext.replace("const ", "").replace("*", "").strip()
                rows.append((i, pname, ctext, ctext.startswith("const "), base if base in names else None))
        out[name] = rows
    return out


def struct_pointers(text):
    """{struct name: [(field, is const, array length or None)]} of the pointer fields of every struct."""
    consts, out = constants(text), {}
    for body, name in re.findall(_STRUCT, _code(text)):
        rows = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.fullmatch(r"((?:const\s+)?\w+)\b\s*(.*)", decl, flags=re.S)
            for declarator in m.group(2).split(","):
                d = re.fullmatch(r"(\**)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?", declarator.strip())
                if d.group(1):
                    n = d.group(3)
                    rows.append((d.group(2), m.group(1).startswith("const"), None if n is None else int(n) if n.isdigit() else consts[n]))
        out[name] = rows
    return out


def _tn(t):
    return getattr(t, "__name__", repr(t))


def signature_mismatches(text, table):
    """What differs between the header's prototypes and a `name -> (restype, [argtypes])` table; every line names the symbol."""
    protos = {name: (res, args) for name, res, args in prototypes(text)}
    out = [f"{n}: declared in the header, not in the table" for n in protos if n not in table]
    out += [f"{n}: in the table, not declared in the header" for n in table if n not in protos]
    for n in protos.keys() & table.keys():
        (hres, hargs), (tres, targs) = protos[n], table[n]
        if hres is not tres:
            out.append(f"{n}: result {_tn(hres)} in the header, {_tn(tres)} in the table")
        if list(hargs) != list(targs):
            out.append(f"{n}: arguments ({', '.join(map(_tn, hargs))}) in the header, ({', '.join(map(_tn, targs))}) in the table")
    if list(protos) != [n for n in table if n in protos] and not out:
        out.append("the table is not in header order")
    return out


def ctypes_fields(cls):
    """[(field, element ctypes type, array length or None)] of a ctypes.Structure"""
    return [(n, t._type_, t._length_) if issubclass(t, C.Array) else (n, t, None) for n, t in cls._fields_]


def struct_mismatches(text, registry):
    """What differs between the header's structs and a `struct name -> ctypes.Structure` registry; every line names the struct."""
    hdr = structs(text)
    out = [f"{n}: defined in the header, not in the registry" for n in hdr if n not in registry]
    out += [f"{n}: in the registry, not defined in the header" for n in registry if n not in hdr]
    for n in hdr.keys() & registry.keys():
        mine = ctypes_fields(registry[n])
        for i, (h, m) in enumerate(zip(hdr[n], mine)):
            if h != m:
                out.append(f"{n}: field {i} is {h[0]} ({_tn(h[1])}, length {h[2]}) in the header, {m[0]} ({_tn(m[1])}, length {m[2]}) "
                           f"in {registry[n].__name__}")
        if len(hdr[n]) != len(mine):
            out.append(f"{n}: {len(hdr[n])} fields in the header, {len(mine)} in {registry[n].__name__}")
    return out


def layout_probe_source(text):
    """A C program that prints `struct size` and `struct.field offset` lines for every struct of the header."""
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "unimm_hip.h"', "int main(void) {"]
    for name, fields in structs(text).items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _, _ in fields]
    return "\n".join(lines + ["  return 0;", "}", ""])
