"""The C ABI of librefnerf_hip.so as ctypes, read from include/refnerf_hip.h: the header is the single source.

parse(text, structs=None, constants=None) -> (constants, structs, prototypes):
  constants   {name: int}: every `#define REFNERF_* <integer expression>` and every enumerator;
  structs     {name: ctypes.Structure subclass}: every `typedef struct`, in header order;
  prototypes  {name: (restype, [argtypes])}: every function.
The parser is strict: comments, the include guard, #include and the `extern "C"` bracket are dropped on purpose, and
whatever else it does not understand raises HeaderError with the offending text -- nothing is skipped.
`structs` and `constants` seed the tables with what an included header declared: parse itself opens no file, so a text that
says `#include "sibling.h"` and names the sibling's types needs them.  load(path) does that: it parses every quoted include
(a header in the same directory) first, seeds the includer with its structs and constants, and returns the includer's own
prototypes -- an entry belongs to the header that declares it.
"""
import ctypes as C
import os
import re

HEADER = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "refnerf_hip.h"))


class HipLibraryError(RuntimeError):
    pass


class HeaderError(HipLibraryError):
    pass


SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double,
           "size_t": C.c_size_t}
_TOKEN = re.compile(r"\s*(0[xX][0-9a-fA-F]+|\d+|[A-Za-z_]\w*|<<|[-+*|()])")
_DECLARATOR = re.compile(r"(\**)\s*(\w+)\s*(?:\[([^\]]*)\])?$")           # [*...] name [[bound]]
_TYPED = re.compile(r"(const\s+)?(\w+)\b\s*(.*)$", re.S)                  # [const] base, then the declarator(s)


def _int(expr, constants):
    """An integer expression over literals, earlier constants and + - * << | ( )."""
    tokens, pos = [], 0
    while pos < len(expr.rstrip()):
        m = _TOKEN.match(expr, pos)
        if not m:
            raise HeaderError(f"not an integer constant expression: {expr.strip()!r}")
        tokens.append(m.group(1))
        pos = m.end()
    try:
        value = eval(" ".join(tokens), {"__builtins__": {}}, dict(constants))
    except Exception:
        value = None
    if not tokens or not isinstance(value, int):
        raise HeaderError(f"not an integer constant expression: {expr.strip()!r}")
    return value


def _ctype(const, base, stars, structs, text):
    """The type map: scalars and structs by value; struct pointers typed, `const char *` a string, any other pointer void*."""
    known = base in SCALARS or base in structs or (base in ("void", "char") and stars)
    if not known:
        raise HeaderError(f"unknown type {base!r} in {text!r}")
    if not stars:
        return SCALARS.get(base) or structs[base]
    if base in structs and stars == "*":
        return C.POINTER(structs[base])
    return C.c_char_p if (const, base, stars) == (True, "char", "*") else C.c_void_p


def _declarations(text, constants, structs, arrays=True):
    """`[const] base declarator {, declarator}` -> [(name, ctype)]; a declarator is `*... name [bound]` (a name is required)."""
    m = _TYPED.match(text)
    if not m:
        raise HeaderError(f"cannot parse the declaration {text!r}")
    out = []
    for decl in m.group(3).split(","):
        d = _DECLARATOR.match(decl.strip())
        if not d or d.group(2) == "const" or (d.group(3) is not None and not arrays):
            raise HeaderError(f"cannot parse the declarator {decl.strip()!r} of {text!r}")
        t = _ctype(bool(m.group(1)), m.group(2), d.group(1), structs, text)
        out.append((d.group(2), t if d.group(3) is None else t * _int(d.group(3), constants)))
    return out


def parse(text, structs=None, constants=None):
    constants, structs, prototypes = dict(constants or {}), dict(structs or {}), {}
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus\b.*?#endif", " ", text, flags=re.S)       # the extern "C" bracket
    # declarations end at a `;` outside braces; preprocessor lines stand alone.  Both kinds keep their order, so that an
    # expression or a member may name whatever came before it
    items, depth, cur = [], 0, ""
    for line in text.split("\n"):
        if line.lstrip().startswith("#"):
            if cur.strip():
                raise HeaderError(f"a preprocessor line inside the declaration {cur.strip()!r}")
            items.append(line.strip())
            continue
        for part in re.split(r"([{};])", line + " "):
            depth += (part == "{") - (part == "}")
            if part == ";" and depth == 0:
                items.append(" ".join(cur.split()))
                cur = ""
            else:
                cur += part
    if cur.strip():
        raise HeaderError(f"unterminated declaration {cur.strip()!r}")
    for item in items:
        if item.startswith("#"):
            m = re.match(r"#\s*define\s+(\w+)\s+(\S.*)$", item)
            if m:
                constants[m.group(1)] = _int(m.group(2), constants)
            elif not re.match(r"#\s*(ifndef\s+\w+|define\s+\w+|endif|include\s*<\w+\.h>|include\s*\"\w+\.h\")$", item):
                raise HeaderError(f"unsupported preprocessor line {item!r}")
            continue
        m = re.match(r"enum \{(.*)\}$", item)
        if m:
            nxt = 0
            for e in m.group(1).strip().rstrip(",").split(","):
                name, _, expr = (s.strip() for s in e.partition("="))
                if not re.match(r"[A-Za-z_]\w*$", name):
                    raise HeaderError(f"cannot parse the enumerator {e.strip()!r}")
                constants[name] = nxt = _int(expr, constants) if expr else nxt
                nxt += 1
            continue
        m = re.match(r"typedef struct (\w+) \{(.*)\} (\w+)$", item)
        if m:
            if m.group(1) != m.group(3) or "{" in m.group(2) or not m.group(2).rstrip().endswith(";"):
                raise HeaderError(f"unsupported struct declaration {item!r}")
            fields = [f for member in m.group(2).split(";")[:-1] for f in _declarations(member.strip(), constants, structs)]
            structs[m.group(1)] = type(m.group(1), (C.Structure,), {"_fields_": fields})
            continue
        m = re.match(r"(const\s+)?(\w+)\s*(\**)\s*\b(\w+)\s*\(([^()]*)\)$", item)
        if not m:
            raise HeaderError(f"unsupported declaration {item!r}")
        restype = None if (m.group(2), m.group(3)) == ("void", "") else _ctype(bool(m.group(1)), m.group(2), m.group(3), structs, item)
        params = [] if m.group(5).strip() == "void" else [_declarations(p.strip(), constants, structs, arrays=False)[0][1] for p in m.group(5).split(",")]
        prototypes[m.group(4)] = (restype, params)
    return constants, structs, prototypes


_loaded = {}       # normalised path -> what load() parsed: a struct is one ctypes class, whichever header's load reaches it


def load(path=HEADER, _including=()):
    if not os.path.exists(path):
        raise HipLibraryError(f"{path} is missing: the ctypes binding is read from the C header")
    path = os.path.normpath(os.path.abspath(path))
    if path in _including:
        raise HeaderError(f"{path} includes itself")
    if path not in _loaded:
        with open(path) as f:
            text = f.read()
        constants, structs = {}, {}
        for name in re.findall(r'^[ \t]*#\s*include\s*"(\w+\.h)"', re.sub(r"/\*.*?\*/", " ", text, flags=re.S), flags=re.M):
            c, s, _ = load(os.path.join(os.path.dirname(path), name), _including + (path,))
            constants.update(c)
            structs.update(s)
        _loaded[path] = parse(text, structs, constants)
    return tuple(dict(table) for table in _loaded[path])


constants, structs, prototypes = load()
