"""The ctypes binding is derived from include/pqlk.h (pql_amd/_lib.py `parse_header`): the type law and the grammar on inline
snippets, then the real header -- the entries where a wrong class corrupts values without a fault are pinned in full, written
from the header by hand.  No kernel is launched here."""
import ctypes as C
import os
import re

import pytest

from pql_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I32, I64, U32, U64, F, D = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_double


def protos(text):
    return L.parse_header(text)[2]


# ---- snippets: the type law ----------------------------------------------------------------------------------------------------
def test_scalar_types_map_by_name():
    got = protos("int pqlk_a(int a, int32_t b, int64_t c, uint32_t d, uint64_t e, float f, double g);\n"
                 "int64_t pqlk_b(int64_t n);\nint32_t pqlk_c(int32_t n);\nvoid pqlk_d(float x);")
    assert got == {"pqlk_a": (C.c_int, [C.c_int, I32, I64, U32, U64, F, D]), "pqlk_b": (I64, [I64]), "pqlk_c": (I32, [I32]),
                   "pqlk_d": (None, [F])}
    assert list(got) == ["pqlk_a", "pqlk_b", "pqlk_c", "pqlk_d"]   # header order


def test_pointers_const_or_not_and_the_stream():
    got = protos("typedef void* pqlk_stream_t;\n"
                 "int pqlk_a(const float* a, float* b, const int64_t *c, int32_t * d, const void* e, uint8_t* f, const uint16_t* g,\n"
                 "           double* h, pqlk_stream_t s);")
    assert got["pqlk_a"] == (C.c_int, [P] * 9)
    with pytest.raises(ImportError, match="pqlk_stream_t"):   # not a type until the header defines it
        protos("int pqlk_a(pqlk_stream_t s);")


def test_struct_pointer_and_char_return():
    consts, structs, got = L.parse_header("typedef struct { int32_t n; } PqlThing;\n"
                                          "int pqlk_a(const PqlThing* a, PqlThing* b);\nconst char* pqlk_name(int rc);")
    assert got["pqlk_a"] == (C.c_int, [C.POINTER(structs["PqlThing"])] * 2)
    assert got["pqlk_name"] == (C.c_char_p, [C.c_int])
    with pytest.raises(ImportError, match="char"):   # c_char_p is a return type only
        protos("int pqlk_a(const char* s);")


def test_void_list_split_lines_and_comments():
    assert protos("int32_t pqlk_a(void);\nint pqlk_b( void );") == {"pqlk_a": (I32, []), "pqlk_b": (C.c_int, [])}
    assert protos("int pqlk_a(const float* x, int64_t ld,\n           float* y /*host*/,\n           double lr);") == {"pqlk_a": (C.c_int, [P, I64, P, D])}
    assert protos("/* call pqlk_x(1); first,\n * then int pqlk_y(int a); */\nint pqlk_z(int a);") == {"pqlk_z": (C.c_int, [C.c_int])}


def test_the_real_header_frame_is_consumed():
    text = ("/* c */\n#ifndef PQLK_H\n#define PQLK_H\n\n#include <stdint.h>\n\n#ifdef __cplusplus\nextern \"C\" {\n#endif\n"
            "int pqlk_a(void);\n#ifdef __cplusplus\n}\n#endif\n#endif /* PQLK_H */\n")
    assert L.parse_header(text) == ({}, {}, {"pqlk_a": (C.c_int, [])})


# ---- snippets: constants and structs -------------------------------------------------------------------------------------------
def test_defines_and_enums():
    consts = L.parse_header("#define PQLK_VERSION 100 /* 0.1.0 */\n#define PQLK_MASK 0x10\n#define PQLK_ROWS(r) (((r) & 15) << 8)\n"
                            "enum { PQLK_A = 0, PQLK_B = 5 };\nenum {\n  PQLK_OK = 0,\n  PQLK_E_NULL = 1 /* why */\n};")[0]
    assert consts == {"VERSION": 100, "MASK": 16, "A": 0, "B": 5, "OK": 0, "E_NULL": 1}
    with pytest.raises(ImportError, match="PQLK_B"):   # values are never counted up by the parser
        L.parse_header("enum { PQLK_A = 0, PQLK_B };")
    with pytest.raises(ImportError, match="PQLK_HALF"):
        L.parse_header("#define PQLK_HALF 0.5f")


def test_struct_fields_and_array_sizes():
    _, structs, _ = L.parse_header("#define PQLK_MAX_LAYERS 8\n"
                                   "typedef struct Tagged {\n  const void* v; /* (N) */\n  float* acc;\n  int64_t n;\n"
                                   "  int32_t dims[PQLK_MAX_LAYERS + 1];\n  float w[2 * (PQLK_MAX_LAYERS - 6)];\n} Tagged;")
    f = structs["Tagged"]._fields_
    assert [n for n, _ in f] == ["v", "acc", "n", "dims", "w"] and [t for _, t in f[:3]] == [P, P, I64]
    assert (f[3][1]._type_, f[3][1]._length_, f[4][1]._type_, f[4][1]._length_) == (I32, 9, F, 4)
    assert issubclass(structs["Tagged"], C.Structure) and C.sizeof(structs["Tagged"]) == 24 + 36 + 16 + 4   # 4: tail pad to 8
    with pytest.raises(ImportError, match="PQLK_NOPE"):
        L.parse_header("typedef struct { int32_t d[PQLK_NOPE]; } PqlT;")
    with pytest.raises(ImportError, match="size_t"):
        L.parse_header("typedef struct { size_t n; } PqlT;")


# ---- snippets: what the parser refuses -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("text, quoted", [
    ("int pqlk_a(const float* x, size_t n);", "size_t n"),
    ("int pqlk_a(PqlNope* p);", "PqlNope"),
    ("int pqlk_a(long n);", "long n"),
    ("size_t pqlk_a(int n);", "size_t pqlk_a"),
    ("int pqlk_a(uint8_t byte);", "uint8_t byte"),
    ("int pqlk_a(unsigned int n);", "unsigned int n"),
    ("int pqlk_a(int);", "pqlk_a(int)"),
    ("int pqlk_a();", "pqlk_a()"),
    ("int pqlk_a(int n); stray", "stray"),
    ("static int pqlk_a(int n);", "static"),
    ("int other_name(int n);", "other_name"),
    ("#define PQLK_X 1\n#pragma once", "#pragma once"),
    ("struct PqlOpen;", "struct PqlOpen"),
])
def test_unknown_text_is_an_import_error_that_quotes_it(text, quoted):
    with pytest.raises(ImportError, match=re.escape(quoted)):
        L.parse_header(text)


def test_missing_header_names_its_path(tmp_path):
    missing = tmp_path / "include" / "pqlk.h"
    with pytest.raises(ImportError, match=re.escape(os.fspath(missing))):
        L.load_header(missing)
    assert os.fspath(L.HEADER_FILE) == os.path.join(ROOT, "include", "pqlk.h")


# ---- the real header -----------------------------------------------------------------------------------------------------------
def test_every_declared_entry_is_bound_once():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pqlk.h")).read(), flags=re.S)
    names = re.findall(r"\b(pqlk_[a-z0-9_]+)\s*\(", text)
    assert len(L.PROTOTYPES) == len(names) and list(L.PROTOTYPES) == names
    for name, (res, args) in L.PROTOTYPES.items():
        fn = getattr(L.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_entries_where_a_wrong_class_corrupts_silently():
    PD, PR = C.POINTER(L.PqlMlpDesc), C.POINTER(L.PqlReplayDesc)
    pins = {
        "pqlk_gae": [P] * 6 + [I32, I64, D, D, I32, P, P, P],
        "pqlk_philox_draws": [U64, I64, I32, P, I64, P, I64, P, I64, I32, I32, P],
        "pqlk_clip_adamw_polyak": [P] * 5 + [I64, F, F] + [D] * 6 + [P] * 4,
        "pqlk_clip_adamw_polyak_pack": [PD] + [P] * 7 + [F, F] + [D] * 6 + [P] * 4,
        "pqlk_adamw_polyak_fused": [PD] + [P] * 7 + [F, F] + [D] * 6 + [P] * 3 + [I32, P, I32, F, P, I32, P],
        "pqlk_synth_env_step": [I64, I32, I32, U32, U32, U32, F] + [P] * 5,
        "pqlk_replay_gather_fused": [PR, P, I64, P, P, F, C.c_int, P, I64, P, P, I64, P, P, P],
        "pqlk_nstep_push_emit": [P, I64, I32, I32, I32, I64, I64] + [P] * 13,
    }
    for name, args in pins.items():
        assert L.PROTOTYPES[name] == (C.c_int, args), name


def test_structs():
    assert L.STRUCTS == {"PqlReplayDesc": L.PqlReplayDesc, "PqlMlpDesc": L.PqlMlpDesc, "PqlInfoKey": L.PqlInfoKey}
    assert (C.sizeof(L.PqlReplayDesc), C.sizeof(L.PqlMlpDesc), C.sizeof(L.PqlInfoKey)) == (32, 44, 40)
    assert L.PqlReplayDesc._fields_ == [("records", P), ("capacity", I64), ("obs_dim", I32), ("act_dim", I32), ("rec_ld", I32),
                                        ("obs_dtype", I32)]
    assert [n for n, _ in L.PqlMlpDesc._fields_] == ["n_layers", "n_nets", "dims"]
    dims = L.PqlMlpDesc._fields_[2][1]
    assert L.PqlMlpDesc._fields_[:2] == [("n_layers", I32), ("n_nets", I32)] and (dims._type_, dims._length_) == (I32, 9)
    assert L.PqlInfoKey._fields_ == [("values", P), ("acc", P), ("ring", P), ("ring_ptr", P), ("dtype", I32), ("mode", I32)]


def test_constants():
    assert (L.ACT_NONE, L.ACT_TANH, L.ACT_TANH_NOISE) == (0, 1, 2)
    assert (L.OBS_F32, L.OBS_F16) == (0, 1)
    assert (L.INFO_F32, L.INFO_U8, L.INFO_LAST, L.INFO_ALL_EPISODE, L.INFO_ALL_STEP) == (0, 1, 0, 1, 2)
    assert (L.MAX_LAYERS, L.INFO_MAX_KEYS, L.C51_MAX_ATOMS, L.QR_MAX_QUANTILES) == (8, 8, 256, 64)
    assert (L.GATHER_CLAMP5, L.GATHER_PADS_ZERO, L.STASH_OUTPUT_ONLY) == (1, 2, 2)
    assert (L.OK, L.E_NULL, L.E_SHAPE, L.E_RANGE, L.E_ALIGN, L.E_UNSUPPORTED, L.E_WORKSPACE) == (0, 1, 2, 3, 4, 5, 6)
    assert L.VERSION == L.lib.pqlk_version() == 100
    assert not hasattr(L, "GATHER_ROWS_IN_FLIGHT") and not hasattr(L, "H")   # function-like macros and the guard are no constants
