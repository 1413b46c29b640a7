"""The ctypes binding is derived from include/virnet_hip.h (virnet_amd/_native.py: parse_header): the reader on small C snippets -- one
accepted example per construct of its subset, one refusal per construct outside it, each naming the line -- then the real header, and
the struct layouts against what the host C compiler says about the same header.  Host only."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from virnet_amd import _native
from virnet_amd._native import NativeLibraryError, parse_header


def test_comments_and_preprocessor_lines():
    h = parse_header('/* a\n   block */\n#ifndef VIRNET_X_H\n#define VIRNET_X_H\n#include <stddef.h>\n#include <stdint.h>\n'
                     '#ifdef __cplusplus\nextern "C" {\n#endif\n#define VIRNET_ABI_VERSION 5   /* why */\n#define VIRNET_MASK 0x10 // tail\n'
                     '// int virnet_hidden(void);\n#ifdef __cplusplus\n}\n#endif\n#endif /* VIRNET_X_H */\n')
    assert h.constants == {"ABI_VERSION": 5, "MASK": 16} and not h.structs and not h.symbols


def test_enums():
    h = parse_header("enum { VIRNET_A = 0, VIRNET_B = 1,\n       VIRNET_C = -2 };\nenum { VIRNET_D = 7 };")
    assert h.constants == {"A": 0, "B": 1, "C": -2, "D": 7}


def test_structs():
    h = parse_header("typedef struct virnet_a {\n  const float* x;   /* in */\n  float *y, *z;\n  void* t;\n  int n, h, w;\n  float slope;\n"
                     "  double d; long l; long long ll; unsigned long long u; size_t s;\n} virnet_a;\n"
                     "typedef struct {\n  int kg, nwv;\n} virnet_b;\n"
                     "typedef struct virnet_c { const float* conv_w[5]; float shift[3], scale[3]; } virnet_c;")
    a, b, c = h.structs["virnet_a"], h.structs["virnet_b"], h.structs["virnet_c"]
    assert a._fields_ == [("x", C.c_void_p), ("y", C.c_void_p), ("z", C.c_void_p), ("t", C.c_void_p), ("n", C.c_int), ("h", C.c_int),
                          ("w", C.c_int), ("slope", C.c_float), ("d", C.c_double), ("l", C.c_long), ("ll", C.c_longlong),
                          ("u", C.c_ulonglong), ("s", C.c_size_t)]
    assert b._fields_ == [("kg", C.c_int), ("nwv", C.c_int)]
    assert c._fields_ == [("conv_w", C.c_void_p * 5), ("shift", C.c_float * 3), ("scale", C.c_float * 3)]
    assert issubclass(a, C.Structure) and a.__name__ == "virnet_a"


def test_prototypes():
    h = parse_header("typedef struct virnet_d { int n; } virnet_d;\n"
                     "int virnet_version(void);\nconst char* virnet_error(void);\nvoid virnet_last(int* out4);\n"
                     "size_t virnet_bytes(int n, long hw, long long per, unsigned long long seed, size_t m, float a, double b);\n"
                     "int virnet_run(const virnet_d* d, virnet_d* out, const float* x, const void* const* src,\n"
                     "               float* const* muls, int out[4], const uint8_t* rgb, const int32_t* idx, int64_t* sse,\n"
                     "               const char* tag, const double* taps, virnet_d* const* many, void* stream);")
    d = h.structs["virnet_d"]
    assert h.symbols == [
        ("virnet_version", C.c_int, []), ("virnet_error", C.c_char_p, []), ("virnet_last", None, [C.c_void_p]),
        ("virnet_bytes", C.c_size_t, [C.c_int, C.c_long, C.c_longlong, C.c_ulonglong, C.c_size_t, C.c_float, C.c_double]),
        ("virnet_run", C.c_int, [C.POINTER(d), C.POINTER(d)] + [C.c_void_p] * 11)]


@pytest.mark.parametrize("line, snippet", [
    (2, "int virnet_a(int n);\nint virnet_b(short x);"),                                    # an unknown type
    (3, "typedef struct virnet_s {\n  int a;\n  int b : 3;\n} virnet_s;"),                   # a bit-field
    (4, "typedef struct virnet_p { int n; } virnet_p;\n\ntypedef struct virnet_s {\n  virnet_p inner;\n} virnet_s;"),   # a struct by value
    (2, "\nint virnet_a(int n, void (*done)(int));"),                                       # a function-pointer parameter
    (3, "\n\nint virnet_a(const char* fmt, ...);"),                                         # variadic
    (2, "#define VIRNET_A 1\n#if VIRNET_A\nint virnet_a(void);\n#endif"),                    # a stray #if
    (2, "int virnet_a(void);\nint other_b(void);"),                                         # a prototype outside virnet_*
    (1, "int virnet_a(int);"),                                                              # an unnamed parameter
    (2, "\ntypedef struct virnet_s { union { int a; float b; } u; } virnet_s;"),            # a union
    (1, "typedef struct virnet_s { int (*cb)(int); } virnet_s;"),                           # a function-pointer member
    (1, "float virnet_a(void);"),                                                           # a return type outside the four
    (1, "int virnet_a(void x);"),                                                           # void by value
    (2, "\n#define VIRNET_A (1 << 4)"),                                                     # a constant that is no integer literal
    (2, "enum { VIRNET_A = 0,\n VIRNET_B };"),                                              # an enumerator without a value
    (2, "#define VIRNET_A 1\n#define VIRNET_A 2"),                                         # a constant defined twice
    (3, "#ifdef __cplusplus\nextern \"C\" {\nint virnet_a(void);\n#endif"),                  # code inside the __cplusplus block
])
def test_outside_the_subset_is_refused_with_the_line(line, snippet):
    with pytest.raises(NativeLibraryError, match=rf"^snippet\.h:{line}: "):
        parse_header(snippet, "snippet.h")


def test_missing_header_names_the_path(tmp_path):
    gone = str(tmp_path / "include" / "virnet_hip.h")
    with pytest.raises(NativeLibraryError, match=re.escape(gone)):
        _native.read_header(gone)


def test_whole_header():
    h = _native.HEADER
    again = _native.read_header()                                  # (a second reading builds its own Structure classes)
    assert again.constants == h.constants and list(again.structs) == list(h.structs)
    assert [(n, r, len(a)) for n, r, a in again.symbols] == [(n, r, len(a)) for n, r, a in h.symbols]
    assert _native.HEADER_PATH == os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_native.__file__))), "include", "virnet_hip.h")
    assert len(h.symbols) == len({s[0] for s in h.symbols}) >= 126 and len(h.structs) >= 12
    # every prototype is bound and nothing else is (test_host.py holds the names to the header's text and to the library's exports)
    assert _native.SYMBOLS == h.symbols
    lib = _native.load()
    for name, restype, argtypes in h.symbols:
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # the one mapping rule: a typed pointer names a struct of this header, everything else is a scalar or void*
    scalars = {C.c_int, C.c_float, C.c_double, C.c_long, C.c_longlong, C.c_ulonglong, C.c_size_t, C.c_void_p}
    typed = {C.POINTER(s): name for name, s in h.structs.items()}
    for name, restype, argtypes in h.symbols:
        assert restype in (C.c_int, C.c_size_t, None, C.c_char_p), name
        assert all(a in scalars or a in typed for a in argtypes), name
    assert {typed[a] for _, _, args in h.symbols for a in args if a in typed} <= set(h.structs)
    # the module's names: one class per struct, one attribute per constant
    bound = {v for v in vars(_native).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}
    assert bound == set(h.structs.values())
    for k, v in h.constants.items():
        assert getattr(_native, k) == v, k
    assert {"ABI_VERSION", "EPI_NHWC", "NCHW_ADD", "GAP_KINFO", "PLAN_WX4X1", "TILE_SLOTS", "OPTIM_CHUNK", "LAUNCH_WX4H"} <= set(h.constants)


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof and offsetof of every struct and field the reader found, printed by a C99 program built against the header with the host
    compiler, equal ctypes' numbers."""
    cc = shutil.which(os.environ.get("CC") or "cc")
    if cc is None:
        pytest.skip("no host C compiler ($CC, else cc) on this machine")
    structs = _native.HEADER.structs
    lines, expect = [], []
    for name, cls in structs.items():
        lines.append(f'  printf("%zu\\n", sizeof({name}));')
        expect.append(C.sizeof(cls))
        for field, _ in cls._fields_:
            lines.append(f'  printf("%zu\\n", offsetof({name}, {field}));')
            expect.append(getattr(cls, field).offset)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "virnet_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(_native.HEADER_PATH), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert len(got) == len(expect) >= 162 and got == expect
