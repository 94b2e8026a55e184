"""ctypes loader for libhulc2_amd.so — the only way compute enters the product path.

There is no CPU or eager-PyTorch fallback: if the HIP library is missing or a kernel rejects a call,
the caller gets an exception (the oracle under oracle/ is test infrastructure and is never imported
from here).

include/hulc2_amd.h is the single source of the binding.  Importing this module reads it once and builds, as plain module globals, one
ctypes.Structure per descriptor struct it declares (hulc_gemm_desc -> GemmDesc, hulc_rnn_wave_desc -> RnnWaveDesc, ...) and DEFINES, its
`#define HULC_X <decimal>` constants; load() binds every prototype from the same text.  A missing header therefore fails at import, with
HulcKernelError, not at the first load().
"""
import ctypes
import os
import re
from pathlib import Path

import torch  # noqa: F401  -- must be imported BEFORE the CDLL below: torch ships its own libamdhip64; loading ours first
#                              would bring a second HIP runtime into the process that owns no device context

_LIB_PATH = Path(__file__).resolve().parent / "libhulc2_amd.so"
if os.environ.get("HULC_LIB"):          # A/B measurements: another BUILD of the same library (e.g. the previous commit's), same ABI
    _LIB_PATH = Path(os.environ["HULC_LIB"]).resolve()
_lib = None


class HulcKernelError(RuntimeError):
    pass


def lib_path() -> Path:
    return _LIB_PATH


_HEADER = Path(__file__).resolve().parent.parent / "include" / "hulc2_amd.h"
_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "unsigned long long": ctypes.c_ulonglong}
_RETURNS = {"int": ctypes.c_int, "long": ctypes.c_long, "const char*": ctypes.c_char_p}
_COMMENTS = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_STRUCT = r"typedef\s+struct\b\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;"


def parse_prototypes(text: str) -> dict:
    """{name: (restype, [argtypes])} of every function the header text declares.  Scalars by value keep their C type, anything with a `*` is
    c_void_p (takes an address, None, byref(struct) or a ctypes array).  Strict: a statement that is not a recognised prototype raises."""
    text = _COMMENTS.sub(" ", text)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(_STRUCT, " ", text)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    protos = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if stmt in ("", "}"):                     # (the brace closes extern "C")
            continue
        m = re.fullmatch(r"(const char ?\*|int|long) ?(hulc_[a-z0-9_]+) ?\((.*)\)", stmt)
        if not m:
            raise HulcKernelError(f"include/hulc2_amd.h: cannot bind `{stmt}`")
        argtypes = []
        for par in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
            if "*" in par:
                argtypes.append(ctypes.c_void_p)
                continue
            base = re.fullmatch(r"\s*(?:const )?([a-z ]+?) [A-Za-z_]\w*\s*", par)
            if not base or base.group(1) not in _SCALARS:
                raise HulcKernelError(f"include/hulc2_amd.h: cannot bind parameter `{par.strip()}` of {m.group(2)}")
            argtypes.append(_SCALARS[base.group(1)])
        protos[m.group(2)] = (_RETURNS[m.group(1).replace(" *", "*")], argtypes)
    return protos


def parse_defines(text: str) -> dict:
    """{name: value} of the object-like `#define HULC_X <decimal>` lines of the header text"""
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(HULC_\w+)[ \t]+(\d+)[ \t]*$", _COMMENTS.sub(" ", text), re.M)}


def parse_structs(text: str) -> dict:
    """{Python name: ctypes.Structure subclass} of every `typedef struct [tag] { ... } hulc_NAME;` the header text declares, fields in header
    order; the Python name is NAME in CamelCase.  Fields: the scalars of _SCALARS by value, c_void_p for every declarator with a `*`, and
    `hulc_OTHER name[LEN]`, an array of a struct declared earlier whose LEN is a decimal or a #defined decimal.  Strict: any other field
    (double, char, a struct by value, a bit-field, any other array) and a union raise."""
    text, defines, structs = _COMMENTS.sub(" ", text), parse_defines(text), {}

    def refuse(what):
        raise HulcKernelError(f"include/hulc2_amd.h: cannot bind {what}")

    if re.search(r"\bunion\b", text):
        refuse("a union")
    found = list(re.finditer(_STRUCT, text))
    if len(found) != len(re.findall(r"\btypedef\s+struct\b", text)):
        refuse("a `typedef struct` that is not `typedef struct [tag] { fields } hulc_NAME;`")
    for m in found:
        cname, fields = m.group(2), []
        if not re.fullmatch(r"hulc_[a-z0-9_]+", cname):
            refuse(f"struct `{cname}`")
        for stmt in m.group(1).split(";"):
            stmt = " ".join(stmt.split())
            if not stmt:
                continue
            arr = re.fullmatch(r"(hulc_\w+) (\w+) ?\[ ?(\w+) ?\]", stmt)
            if arr:
                n = int(arr.group(3)) if arr.group(3).isdigit() else defines.get(arr.group(3))
                if arr.group(1) not in structs or not n:
                    refuse(f"field `{stmt}` of {cname}: an array needs an earlier struct and a decimal or #defined length")
                fields.append((arr.group(2), structs[arr.group(1)] * n))
                continue
            first, *more = stmt.split(",")
            head = re.fullmatch(r"(?:const )?([A-Za-z_]\w*(?: [A-Za-z_]\w*)*?) ?(\** ?[A-Za-z_]\w*)", first)
            if not head:
                refuse(f"field `{stmt}` of {cname}")
            for decl in [head.group(2)] + more:
                d = re.fullmatch(r"(\**) ?([A-Za-z_]\w*)", decl.strip())
                if not d or not (d.group(1) or head.group(1) in _SCALARS):
                    refuse(f"field `{stmt}` of {cname}")
                fields.append((d.group(2), ctypes.c_void_p if d.group(1) else _SCALARS[head.group(1)]))
        structs[cname] = type("".join(p.capitalize() for p in cname[5:].split("_")), (ctypes.Structure,),
                              {"_fields_": fields, "__doc__": f"{cname} of include/hulc2_amd.h"})
    return {cls.__name__: cls for cls in structs.values()}


if not _HEADER.exists():
    raise HulcKernelError(f"{_HEADER} is missing: the binding takes every prototype from it")
_HEADER_TEXT = _HEADER.read_text()
DEFINES = parse_defines(_HEADER_TEXT)
TXL_MAX_LAYERS = DEFINES["HULC_TXL_MAX_LAYERS"]
globals().update(parse_structs(_HEADER_TEXT))       # GemmDesc, ConvDesc, MixDesc, TxlAttnDesc, TxlBlockLayer, TxlBlockDesc, MlpChainLayer, ...


def load():
    """Load the shared library once; raise loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise HulcKernelError(
            f"{_LIB_PATH} is missing: build it with `python -m hulc2_amd.build` "
            "(hipcc --offload-arch=gfx950). hulc2_amd has no non-HIP fallback."
        )
    lib = ctypes.CDLL(os.fspath(_LIB_PATH))
    for name, (restype, argtypes) in parse_prototypes(_HEADER_TEXT).items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise HulcKernelError(f"{_LIB_PATH} does not export {name}, which {_HEADER.name} declares: rebuild the library") from None
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().hulc_last_error().decode(errors="replace")
        raise HulcKernelError(f"{what} failed with code {rc}: {msg}")
