"""C-ABI surface checks that need no GPU: the library loads, exports everything include/*.h declares,
sizes its workspaces sanely and reports errors through return codes (never by crashing)."""
import ctypes
import os
import re

import pytest

from adaptigraph_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "adaptigraph_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ag_[a-z0-9_]+)\s*\(", text)))


def declared_prototypes():
    """name -> (return type, [parameter types]) of every function the header declares, as C text without `const` and parameter names;
    a pointer parameter of any kind is "*"."""
    text = open(os.path.join(ROOT, "include", "adaptigraph_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)                 # block comments and the inline /*host*/ ones
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)                  # preprocessor lines
    strip = lambda c: " ".join(w for w in c.replace("*", " * ").split() if w != "const")
    protos = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(ag_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in protos, name
        params = [strip(q) for q in params.split(",")]
        protos[name] = (strip(ret), [] if params == ["void"] else ["*" if "*" in q else q.rsplit(" ", 1)[0] for q in params])
    return protos


C_VALUE_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
                 "ag_stream_t": ctypes.c_void_p}
C_RETURN_TYPES = dict(C_VALUE_TYPES, **{"char *": ctypes.c_char_p, "void": None})


def signature_mismatches(signatures):
    """Where a name -> (restype, [argtypes]) table disagrees with the header's prototypes; [] when every position agrees."""
    bad = []
    protos = declared_prototypes()
    if sorted(protos) != sorted(signatures):
        bad.append(f"names differ: {sorted(set(protos) ^ set(signatures))}")
    for name, (ret, params) in protos.items():
        restype, argtypes = signatures.get(name, (None, []))
        if restype is not C_RETURN_TYPES[ret]:
            bad.append(f"{name}: returns {ret}, table says {restype}")
        if len(argtypes) != len(params):
            bad.append(f"{name}: {len(params)} parameters, table has {len(argtypes)}")
        for i, (c, t) in enumerate(zip(params, argtypes)):
            if c == "*":
                ok = t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))
            else:
                ok = t is C_VALUE_TYPES[c]
            if not ok:
                bad.append(f"{name}: parameter {i} is {'a pointer' if c == '*' else c}, table says {getattr(t, '__name__', t)}")
    return bad


def test_signature_table_matches_the_header_position_by_position():
    """Every row of _lib.SIGNATURES against its prototype in include/adaptigraph_hip.h: the return type, the number of parameters and every
    parameter (int / int64_t / size_t / float by their exact ctypes type, ag_stream_t as c_void_p, any pointer as c_void_p, c_char_p or a
    POINTER type), and the loaded functions carry exactly the table's types.  A wrong count, a pointer where an integer goes (or the
    reverse) and a 32/64-bit swap are each reported, which the corrupted copies below show."""
    assert len(declared_prototypes()) == len(declared_symbols()) >= 48
    assert signature_mismatches(_lib.SIGNATURES) == []
    L = _lib.lib()
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    ret, args = _lib.SIGNATURES["ag_fps"]
    size_at = args.index(ctypes.c_size_t)
    for row, what in (((ret, args[:-1]), "13 parameters, table has 12"),
                      ((ret, args[:size_at] + [ctypes.c_void_p] + args[size_at + 1:]), f"parameter {size_at} is size_t, table says c_void_p"),
                      ((ret, [ctypes.c_size_t] + args[1:]), "parameter 0 is a pointer, table says " + ctypes.c_size_t.__name__),
                      ((ret, args[:3] + [ctypes.c_int64] + args[4:]), "parameter 3 is int, table says " + ctypes.c_int64.__name__),
                      ((ctypes.c_int64, args), "returns int, table says")):
        bad = signature_mismatches(dict(_lib.SIGNATURES, ag_fps=row))
        assert len(bad) == 1 and bad[0].startswith("ag_fps: " + what), (what, bad)


def test_library_exports_every_declared_symbol():
    L = _lib.lib()
    names = declared_symbols()
    assert len(names) >= 12
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/adaptigraph_hip.h but not exported"
    assert sorted(_lib.EXPORTS) == names


def test_dynamic_symbol_table_is_exactly_the_header():
    """-fvisibility=hidden + csrc/exports.map: `nm -D` shows the declared ag_* functions and nothing else (no mangled launchers,
    no template instantiations, no __hip_cuid_* words)."""
    import shutil
    import subprocess
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.check_output([nm, "-D", "--defined-only", _lib.build()], text=True)
    exported = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    assert exported == declared_symbols()


def test_every_engine_option_is_one_table_row_documented_in_the_header():
    """ag_set_option, ag_get_option and ag_model_create's environment all go through one option table (csrc/ag_model.hip: kOptions), one row per
    option (name, environment variable, field, validation), so the names set and get accept are the same by construction; each option and its
    environment variable is described in the header's option list (a caller of the C ABI has nothing else to go by)."""
    src = open(os.path.join(ROOT, "adaptigraph_amd", "csrc", "ag_model.hip")).read()
    table = src[src.index("const Option kOptions[] = {"):src.index("};", src.index("const Option kOptions[] = {"))]
    rows = re.findall(r'\{"([a-z0-9_]+)", "(AG_[A-Z0-9_]+)", &ag_model::[a-z0-9_]+, ', table)
    names, envs = [r[0] for r in rows], [r[1] for r in rows]
    assert len(rows) == table.count('{"') and len(set(names)) == len(names) >= 12 and len(set(envs)) == len(envs)
    for fn in ("ag_set_option", "ag_get_option"):
        body = src[src.index(f"int {fn}("):src.index("return AG_OK;", src.index(f"int {fn}("))]
        assert "find_option(name)" in body and "strcmp" not in body, fn
    header = open(os.path.join(ROOT, "include", "adaptigraph_hip.h")).read()
    for n, e in rows:
        assert f'"{n}"' in header, f"option {n} is not described in include/adaptigraph_hip.h"
        assert e in header, f"environment variable {e} of option {n} is not named in include/adaptigraph_hip.h"


def test_version_and_capacity_queries():
    L = _lib.lib()
    assert L.ag_version() >= 1
    assert L.ag_edge_capacity(256, 1001, 10, 0, 1) == 256 * 1001 * 10
    assert L.ag_edge_capacity(2, 4097, 5, 1, 1) == 2 * 4097 * 6
    assert L.ag_edge_capacity(2, 7, 10, 0, 1) == 2 * 7 * 7          # topk clipped to N (graph.py:128)
    e_cap = 256 * 1001 * 10
    fwd = L.ag_forward_workspace_bytes(256, 1001, e_cap)
    assert fwd >= e_cap * 160 * 4 + 5 * 256 * 1001 * 160 * 4      # Eterm + five node tables
    prm = _lib.RolloutParams(256, 1001, 1000, 1, 10, 0, 1, 10, 0, 0.0)
    assert L.ag_rollout_workspace_bytes(ctypes.byref(prm)) > fwd
    assert L.ag_rollout_workspace_bytes(ctypes.byref(prm)) <= 2.95e9               # bounded compact tables (r05; 3.55 GB until r04); 2.11 GB for a default-mode model
    assert L.ag_rollout_workspace_bytes_for(None, ctypes.byref(prm)) == L.ag_rollout_workspace_bytes(ctypes.byref(prm))   # no model: any mode
    assert L.ag_edges_workspace_bytes(256, 1001, 10, 0, 1) >= 256 * 1001 * 11 * 4


# (B, N, n_p, n_instance, topk, connect_tools_all, max_tools) -> ag_edge_capacity, ag_edges_workspace_bytes, ag_forward_workspace_bytes,
# ag_rollout_workspace_bytes, ag_rollout_scripted_workspace_bytes_for(NULL); n_steps 4, height mode 0, builder variant "batch".
# Recorded from the library before the rollout drivers shared one carving of a step's graph buffers.
WORKSPACE_BYTES = {
    (1, 2, 1, 1, 10, 0, 1): (4, 34560, 4038400, 4075520, 4074752),
    (7, 9, 8, 1, 5, 1, 1): (378, 234496, 4203264, 4446720, 4446464),
    (8, 301, 300, 1, 10, 0, 1): (24080, 408064, 30014208, 30818560, 30827520),
    (16, 301, 300, 1, 20, 0, 1): (96320, 1007360, 87566592, 93209088, 89769216),
    (31, 65, 64, 2, 5, 1, 1): (12090, 1146880, 20847872, 29435904, 22268928),
    (33, 257, 256, 0, 64, 0, 0): (542784, 3424512, 392628992, 412413440, 401142784),
    (256, 1001, 1000, 1, 10, 0, 1): (2562560, 23778304, 2862914816, 2931705856, 2929739264),
    (2, 4101, 4096, 1, 5, 1, 5): (82020, 723200, 94052096, 96122112, 96154112),
}


def workspace_queries(model, B, N, n_p, n_inst, topk, connect, max_tools):
    """The five sizes of one WORKSPACE_BYTES row, for `model` (a handle, or None: any model)."""
    L = _lib.lib()
    e_cap = L.ag_edge_capacity(B, N, topk, connect, max_tools)
    rollout = _lib.RolloutParams(B, N, n_p, n_inst, topk, connect, max_tools, 4, _lib.AG_HEIGHT_MIN, 0.0)
    scripted = _lib.ScriptedParams(B, N, n_p, n_inst, topk, connect, max_tools, _lib.AG_VARIANT_BATCH, 4)
    return (e_cap, L.ag_edges_workspace_bytes(B, N, topk, connect, max_tools), L.ag_forward_workspace_bytes_for(model, B, N, e_cap),
            L.ag_rollout_workspace_bytes_for(model, ctypes.byref(rollout)), L.ag_rollout_scripted_workspace_bytes_for(model, ctypes.byref(scripted)))


def test_model_less_workspace_sizes_are_the_recorded_ones():
    """Every carving of a workspace keeps its offsets: 1 to 4 possible batch parts and the cap B / parts >= 8, edge lists with and without the
    tail of elided self-loops, connect_tools_all, n_instance 0 and 2, and a top-k clipped to N."""
    L = _lib.lib()
    for row, want in WORKSPACE_BYTES.items():
        assert workspace_queries(None, *row) == want, row
        prm = _lib.RolloutParams(*row, 4, _lib.AG_HEIGHT_MIN, 0.0)
        assert L.ag_rollout_workspace_bytes(ctypes.byref(prm)) == want[3], row
        assert L.ag_forward_workspace_bytes(row[0], row[1], want[0]) == want[2], row


def test_errors_are_codes_not_crashes():
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.ag_model_create(None, None, ctypes.byref(h)) != 0
    assert b"null" in L.ag_last_error()
    v = ctypes.c_int(7)
    assert L.ag_get_option(None, b"precision", ctypes.byref(v)) != 0 and b"null" in L.ag_last_error() and v.value == 7
    bad = _lib.ModelConfig(128, 4, 2, 1, 3, 3, 100.0)              # nf the kernels are not built for
    dummy = (ctypes.c_void_p * 22)(*([1] * 22))
    assert L.ag_model_create(ctypes.byref(bad), dummy, ctypes.byref(h)) == -4
    assert b"nf=128" in L.ag_last_error()
    assert L.ag_build_edges(None, None, None, None, 10, 0, 1, 1, 8, 1, None, None, None, 80, None, 0, None) != 0
    assert L.ag_model_destroy(None) == 0


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_LIB", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.lib()


def test_training_entry_points_reject_bad_arguments_without_a_gpu():
    """Argument checks of the row-n4 entry points run before any HIP call: null tables, widths beyond the compiled 150, chain
    kinds / input widths that do not exist, ragged element counts — all come back as AG_ERR_ARG (-1) with a message."""
    L = _lib.lib()
    assert L.ag_train_pack(None, None, 150, 150, 150, 0, 0, 0, 5, 0, None, None) == -1
    buf = (ctypes.c_float * 8)()
    assert L.ag_train_pack(buf, None, 150, 151, 151, 0, 0, 0, 5, 0, buf, None) == -1                 # n_in > 150
    assert L.ag_train_pack(buf, buf, 150, 40, 40, 0, 0, 1, 1, 0, buf, None) == -1                    # compact image holds <= 32 columns
    arr = (ctypes.c_void_p * 4)()
    assert L.ag_train_chain(7, 0, 0, buf, buf, arr, None, arr, None, 10, 17, None) == -1               # unknown kind
    assert L.ag_train_chain(0, 0, 0, buf, buf, arr, None, arr, None, 10, 16, None) == -1               # edge chain takes 17 inputs
    assert L.ag_train_chain(0, 0, 0, buf, buf, arr, None, arr, None, 10, 17, None) == -1               # null layer table
    assert b"table 0" in L.ag_last_error()
    assert L.ag_add3_relu(buf, buf, buf, buf, 6, None) == -1                                           # n % 4 != 0
    assert L.ag_relu_mask(None, buf, buf, 8, None) == -1
    i32 = (ctypes.c_int32 * 4)(160, 0, 0, 0)
    assert L.ag_train_weight_grads(0, arr, i32, arr, i32, i32, 10, buf, buf, 1 << 20, None) == -1      # n_layers < 1
    assert L.ag_train_weight_grads_workspace_bytes(48000, 4) > L.ag_train_weight_grads_workspace_bytes(1000, 1) > 0
    assert L.ag_edge_inputs_forward(buf, 15, 2, 14, None, None, None, 0, None) == -1                   # attr + group > D
    assert L.ag_model_status(None, None, None) == -1
