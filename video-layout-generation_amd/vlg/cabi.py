"""The C ABI as Python sees it, read from include/vlg_hip.h: prototypes as ctypes, parameter names, #define values, enums.

A strict reader of THAT header's grammar (its opening comment lists the rules), not a C parser: anything else raises a
ValueError that quotes the text.  Pure Python - no torch, no loaded library (vlg.spec reads its constants through here).
"""
from __future__ import annotations

import collections
import functools
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_uint32, c_uint64, c_void_p

HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "vlg_hip.h"))
SCALARS = {"int": c_int, "int64_t": c_int64, "uint32_t": c_uint32, "uint64_t": c_uint64, "float": c_float, "double": c_double}
RESTYPES = {"int": c_int, "int64_t": c_int64, "void": None, "const char*": c_char_p}
_POINTEES = frozenset(SCALARS) | {"void", "char", "uint8_t", "uint16_t", "unsigned long long"}   # + what the header typedefs
_NUMBER = re.compile(r"(-?\d+)|\((-?\d+\.\d+)f\)")
_BLOCK = r"\b(typedef\s+struct|enum)\s*(\w*)\s*\{([^{}]*)\}\s*(\w*)\s*;"      # typedef struct [tag] {...} name;  enum name {...};


# functions: name -> (restype, ((ctype, param_name), ...));  diag_functions: the same for the prototypes inside #ifdef VLG_DIAG;
# constants: VLG_X -> int | float;  enums: enum name -> {member: int}
Header = collections.namedtuple("Header", "functions diag_functions constants enums")


def _bad(what: str, text: str) -> ValueError:
    return ValueError("include/vlg_hip.h grammar: %s: %r" % (what, " ".join(text.split())))


def _param(text: str, pointees):
    tok = [t for t in re.findall(r"\w+|\.\.\.|\S", text) if t != "const"]
    name, stars = (tok or [""])[-1], tok.count("*")
    base = " ".join(tok[:-1 - stars])
    named = name.isidentifier() and name not in pointees and name not in ("long", "unsigned") and base
    if not named or tok[-1 - stars:-1] != ["*"] * stars or base not in (pointees if stars else SCALARS):
        raise _bad("parameter must be `<type> name`, the type one of %s or a pointer to a declared type" % ", ".join(SCALARS), text)
    return (c_void_p if stars else SCALARS[base]), name


def _prototype(stmt: str, pointees):
    m = re.fullmatch(r"(const\s+char\s*\*|\w+)\s*\b(\w+)\s*\((.*)\)", stmt, flags=re.S)
    res = re.sub(r"\s*\*", "*", " ".join(m.group(1).split())) if m else None
    if res not in RESTYPES:
        raise _bad("not a prototype returning int, int64_t, void or const char*", stmt)
    params = () if m.group(3).strip() == "void" else tuple(_param(p, pointees) for p in m.group(3).split(","))
    if "stream" in [n for _, n in params[:-1]]:
        raise _bad("`stream` must be the last parameter", stmt)
    return m.group(2), (RESTYPES[res], params)


def parse(text: str) -> Header:
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)                                   # (a // comment ends up refused as a declaration)
    hdr, pointees, seen = Header({}, {}, {}, {}), set(_POINTEES), set()
    body, open_ifs, guard = {False: [], True: []}, [], None      # body[diag]: declaration lines outside / inside VLG_DIAG

    def declare(name, table, value, src):
        if name in seen:
            raise _bad("declared twice", src)
        seen.add(name)
        table[name] = value

    for line in text.splitlines():
        s = " ".join(line.split())
        if not s.startswith("#"):
            if "__cplusplus" not in open_ifs:                    # extern "C" { ... } is the C++ compiler's business
                body["VLG_DIAG" in open_ifs].append(line)
            continue
        word, _, rest = s[1:].strip().partition(" ")
        define = re.fullmatch(r"(VLG_\w+) (.+)", rest) if word == "define" else None
        number = _NUMBER.fullmatch(define.group(2)) if define else None
        if word == "ifndef" and guard is None and rest.isidentifier():
            guard = rest                                         # the include guard: the one #ifndef, closed by `#define <guard>`
            open_ifs.append(rest)
        elif word == "ifdef" and rest in ("__cplusplus", "VLG_DIAG"):
            open_ifs.append(rest)
        elif word == "endif" and not rest and open_ifs:
            open_ifs.pop()
        elif number:
            declare(define.group(1), hdr.constants, float(number.group(2)) if number.group(1) is None else int(number.group(1)), s)
        elif not ((word == "include" and rest == "<stdint.h>") or (word == "define" and rest == guard)):
            raise _bad("preprocessor line (allowed: the include guard, #include <stdint.h>, #ifdef __cplusplus | VLG_DIAG, "
                       "#endif, #define VLG_NAME <number>)", s)
    if open_ifs:
        raise _bad("#if without #endif", open_ifs[-1])

    for diag, table in ((False, hdr.functions), (True, hdr.diag_functions)):
        decls = "\n".join(body[diag])
        for kind, tag, inside, name in re.findall(_BLOCK, decls):
            members = [re.fullmatch(r"\s*(\w+)\s*=\s*(-?\d+)\s*", item) for item in inside.split(",")]
            if kind != "enum":
                pointees.add(name)
            elif not all(members):
                raise _bad("enum member without an explicit value", inside)
            else:
                declare(tag, hdr.enums, {m.group(1): int(m.group(2)) for m in members}, "enum " + tag)
        *stmts, tail = (d.strip() for d in re.sub(_BLOCK, "", decls).split(";"))
        if tail:
            raise _bad("declaration without its `;`", tail)
        for stmt in filter(None, stmts):
            m = re.fullmatch(r"typedef\s+(\w+)\s+(\w+)", stmt)
            if m and m.group(1) in pointees:
                pointees.add(m.group(2))
            else:
                name, signature = _prototype(stmt, pointees)
                declare(name, table, signature, stmt)
    return hdr


@functools.lru_cache(maxsize=None)
def header() -> Header:
    """include/vlg_hip.h of this tree, parsed once per process (OSError if the file is missing)"""
    with open(HEADER_PATH) as f:
        return parse(f.read())


def values(prefix: str, *names: str) -> tuple:
    """header().constants[prefix + name] for each name: binds a group of module-level names in one statement"""
    return tuple(header().constants[prefix + n] for n in names)
