"""ctypes binding of ``libvirnet_hip.so``, derived from the C ABI's one declaration, ``include/virnet_hip.h``.

The header is read once at import (``read_header``): its prototypes become ``SYMBOLS``, its structs the Structure classes below, its
integer constants module attributes without the ``VIRNET_`` prefix.  The reader takes exactly the C subset the header uses (DESIGN.md
names it) and refuses anything else with the line number, so a header edit it cannot follow fails on the host, never in a launch.

There is no CPU fallback: if the library is missing or a call fails this module raises.
``import torch`` happens first on purpose -- PyTorch-ROCm ships its own ``libamdhip64.so.7``; loading it first
makes our library bind to the same HIP runtime instance, so torch's device pointers and stream handles are
valid inside our launches.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import threading
from typing import NamedTuple

import torch  # noqa: F401  (must precede CDLL, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
# VIRNET_HIP_LIB lets a tuning run point at another in-tree build of the same ABI (A/B kernel experiments)
LIB_PATH = os.environ.get("VIRNET_HIP_LIB") or os.path.join(_HERE, "lib", "libvirnet_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "virnet_hip.h")


class NativeLibraryError(RuntimeError):
    pass


class Header(NamedTuple):
    constants: dict      # "EPI_NHWC" -> 0: every #define / enum constant, without the VIRNET_ prefix
    structs: dict        # "virnet_conv_desc" -> its ctypes.Structure class
    symbols: list        # (name, restype, argtypes) per prototype, in header order


_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "long": C.c_long, "long long": C.c_longlong,
            "unsigned long long": C.c_ulonglong, "size_t": C.c_size_t}
_POINTEES = {"uint8_t", "int32_t", "int64_t", "char", "void"}        # known behind a pointer only
_RESTYPES = {"int": C.c_int, "size_t": C.c_size_t, "void": None, "const char*": C.c_char_p}
_SPACE = re.compile(r"\s*")
_INT = r"(-?(?:0[xX][0-9a-fA-F]+|\d+))"
_ENUM = re.compile(r"enum\s*\{([^{}]*)\}\s*;")
_STRUCT = re.compile(r"typedef\s+struct\s*(\w+)?\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTO = re.compile(r"([\w\s*]*?)(\w+)\s*\(([^;{}]*)\)\s*;")
_BASE = re.compile(r"\s*(?:const\s+)?(unsigned\s+long\s+long|long\s+long|\w+)\b(.*)", re.S)
_DECLARATOR = re.compile(r"\s*((?:\*\s*(?:const\b\s*)?)*)([A-Za-z_]\w*)\s*(?:\[\s*(\d+)\s*\])?\s*")


def parse_header(text: str, where: str = "header") -> Header:
    """The constants, structs and prototypes of a header written in the subset virnet_hip.h uses; NativeLibraryError otherwise."""
    def fail(pos, msg):
        raise NativeLibraryError(f"{where}:{text.count(chr(10), 0, pos) + 1}: {msg}")

    def pieces(m, group, sep):
        """The `sep`-separated pieces of a match's group, each with the offset of its first character that is no blank."""
        at = m.start(group)
        for piece in m.group(group).split(sep):
            yield piece, at + len(piece) - len(piece.lstrip())
            at += len(piece) + 1

    def declarations(decl, pos, member):
        """`const float *a, *b[5]` -> [(name, ctype), ...]; the one rule that maps a C declaration to ctypes."""
        base = _BASE.fullmatch(decl)
        kind = " ".join(base.group(1).split()) if base else ""
        if kind not in _SCALARS and kind not in _POINTEES and kind not in structs:
            fail(pos, f"unknown type in `{' '.join(decl.split())}`")
        out = []
        for d in base.group(2).split(","):
            m = _DECLARATOR.fullmatch(d)
            if not m:
                fail(pos, f"unsupported declarator `{' '.join(decl.split())}`")
            stars, length = m.group(1).count("*"), m.group(3)
            if stars == 0 and kind not in _SCALARS:
                fail(pos, f"`{kind} {m.group(2)}`: {kind} is known behind a pointer only")
            if member:
                t = C.c_void_p if stars else _SCALARS[kind]
                t = t * int(length) if length else t
            elif stars == 1 and not length and kind in structs:
                t = C.POINTER(structs[kind])
            else:
                t = C.c_void_p if stars or length else _SCALARS[kind]
            out.append((m.group(2), t))
        return out

    constants, structs, symbols = {}, {}, []
    # a comment becomes a blank and its newlines, a directive is checked and blanked: line numbers stay those of the file
    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: " " + "\n" * m.group().count("\n"), text, flags=re.S)

    def constant(name, value, pos):
        if not name.startswith("VIRNET_") or name[7:] in constants:
            fail(pos, f"constant {name}: not VIRNET_*, or defined twice")
        constants[name[7:]] = int(value, 0)

    depth, guard, in_cxx, pos, lines = 0, None, False, 0, text.split("\n")
    for i, line in enumerate(lines):
        s = " ".join(line.split())
        if s.startswith("#"):
            s = re.sub(r"^# ", "#", s)
            define = re.fullmatch(r"#define (\w+) " + _INT, s)
            if re.fullmatch(r"#ifndef \w+", s) and guard is None and depth == 0:
                guard, depth = s.split()[1], 1
            elif s == f"#define {guard}" and depth == 1:
                pass
            elif s in ("#include <stddef.h>", "#include <stdint.h>"):
                pass
            elif s == "#ifdef __cplusplus" and not in_cxx:
                in_cxx, depth = True, depth + 1
            elif s == "#endif" and depth > 0:
                in_cxx, depth = False, depth - 1
            elif define:
                constant(define.group(1), define.group(2), pos)
            else:
                fail(pos, f"unsupported preprocessor line `{s}`")
            lines[i] = ""
        elif in_cxx:
            if s not in ('extern "C" {', "}", ""):
                fail(pos, f"unsupported line under #ifdef __cplusplus: `{s}`")
            lines[i] = ""
        pos += len(line) + 1
    if depth:
        fail(len(text), "unterminated #if")
    text = "\n".join(lines)

    pos = _SPACE.match(text).end()
    while pos < len(text):
        if m := _ENUM.match(text, pos):
            for item, at in pieces(m, 1, ","):
                e = re.fullmatch(r"\s*(\w+)\s*=\s*" + _INT + r"\s*", item)
                if not e:
                    fail(at, f"unsupported enumerator `{' '.join(item.split())}`")
                constant(e.group(1), e.group(2), at)
        elif m := _STRUCT.match(text, pos):
            name, fields = m.group(3), []
            if m.group(1) not in (None, name) or name in structs or not name.startswith("virnet_"):
                fail(pos, f"struct {name}: tag and name differ, not virnet_*, or defined twice")
            for decl, at in pieces(m, 2, ";"):
                if decl.strip():
                    fields += declarations(decl, at, member=True)
            structs[name] = type(name, (C.Structure,), {"_fields_": fields, "__doc__": f"{name} ({where})"})
        elif m := _PROTO.match(text, pos):
            ret, name, params = " ".join(m.group(1).split()).replace(" *", "*"), m.group(2), m.group(3)
            if ret not in _RESTYPES or not name.startswith("virnet_") or name in {s[0] for s in symbols}:
                fail(pos, f"`{ret} {name}(..)`: returns none of int, size_t, void, const char*; or is not virnet_*; or is declared twice")
            argtypes = []
            for p, at in ([] if params.strip() == "void" else pieces(m, 3, ",")):
                argtypes += [t for _, t in declarations(p, at, member=False)]
            symbols.append((name, _RESTYPES[ret], argtypes))
        else:
            fail(pos, f"unsupported declaration `{' '.join(text[pos:pos + 60].split())} ..`")
        pos = _SPACE.match(text, m.end()).end()
    return Header(constants, structs, symbols)


def read_header(path: str | None = None) -> Header:
    path = path or HEADER_PATH
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise NativeLibraryError(f"{path}: cannot read the C ABI's header, which the binding is derived from ({e})") from e
    return parse_header(text, os.path.relpath(path, os.path.dirname(_HERE)) if path == HEADER_PATH else path)


HEADER = read_header()


def _struct(cname: str) -> type:
    return HEADER.structs[cname]


ConvPlan = _struct("virnet_conv_plan")
ConvDesc = _struct("virnet_conv_desc")
ConvLaunch = _struct("virnet_conv_launch")
WgradF16Plan = _struct("virnet_wgrad_f16_plan")
TEmit = _struct("virnet_t_emit")
PackDesc = _struct("virnet_pack_desc")
ImageGradDesc = _struct("virnet_image_grad_desc")
ThinDesc = _struct("virnet_thin_desc")
WgradDesc = _struct("virnet_wgrad_desc")
KnetLayer = _struct("virnet_knet_layer")
SftWeights = _struct("virnet_sft_weights")
LpipsWeightsDesc = _struct("virnet_lpips_weights")

# every integer constant of the header, VIRNET_ dropped: ABI_VERSION, EPI_NHWC, NCHW_ADD, GAP_KINFO, PLAN_WX4X1, LAUNCH_WX4H, OPTIM_CHUNK, ...
if set(HEADER.constants) & set(globals()):
    raise NativeLibraryError(f"{HEADER_PATH}: constants that collide with names of the binding: {sorted(set(HEADER.constants) & set(globals()))}")
globals().update(HEADER.constants)

# every symbol include/virnet_hip.h declares: (name, restype, argtypes)
SYMBOLS = HEADER.symbols

_lib = None


def load() -> C.CDLL:
    """Load (once) and type the library; raise loudly when it is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} not found: the VIRNet HIP kernels are not built. Run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (or `make -C virnet_amd/csrc`) -- there is no CPU fallback for the product path.")
    lib = C.CDLL(LIB_PATH)
    for name, restype, argtypes in SYMBOLS:
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise NativeLibraryError(f"{LIB_PATH} does not export {name}; rebuild it") from e
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.virnet_abi_version() != ABI_VERSION:  # noqa: F821  (from the header, see above)
        raise NativeLibraryError(f"{LIB_PATH}: ABI {lib.virnet_abi_version()} != expected {ABI_VERSION}; rebuild it")  # noqa: F821
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().virnet_last_error()
        raise RuntimeError(f"libvirnet_hip {what}: {msg.decode() if msg else 'unknown error'}")


def ptr(t) -> int:
    """Device address of a tensor (0 for None)."""
    return 0 if t is None else t.data_ptr()


tls = threading.local()      # ops.forward_scope keeps its per-forward snapshot here (stream handle, environment knobs): one per host thread
# Held by every hipGraph capture of this package (graph.py) and by the few host calls that HIP does not permit while ANY stream of the
# process is capturing -- pinned-memory allocation, destruction of a captured graph -- even from another thread in thread-local capture
# mode (tools/probes/capture_concurrency.py): one of those at the wrong moment invalidates the other thread's capture.
capture_lock = threading.RLock()


def stream_handle() -> int:
    """hipStream_t of torch's current stream, as the void* the C ABI takes."""
    cached = getattr(tls, "stream_cache", None)
    if cached is not None:
        return cached
    return torch.cuda.current_stream().cuda_stream
