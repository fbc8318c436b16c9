"""Host-side checks of the batched greedy loop (no GPU): include/tgnn.h declares the four `_many` entries with the argument
lists tilingnn_amd/_lib.py binds, the public functions exist with their documented signatures, and bad arguments are rejected
before anything is launched."""
import ctypes as C
import inspect
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("tgnn_sublayout_compact_many", "tgnn_greedy_round_many", "tgnn_greedy_finish_many", "tgnn_solution_score_sums_many",
           "tgnn_sublayout_compact_many_workspace_bytes", "tgnn_greedy_round_many_workspace_bytes",
           "tgnn_solution_score_sums_many_workspace_bytes")


def _declarations():
    text = open(os.path.join(REPO, "include", "tgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(2): (m.group(1).strip(), [a.strip() for a in m.group(3).split(",")])
            for m in re.finditer(r"\b(int|size_t|int64_t)\s+(tgnn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def _ctype_of(arg):
    if "*" in arg:
        return C.c_void_p
    kind = arg.rsplit(" ", 1)[0].replace("const ", "").strip()
    return {"int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "tgnn_stream_t": C.c_void_p, "float": C.c_float}[kind]


def test_header_and_binding_table_agree_on_the_many_entries():
    from tilingnn_amd import _lib
    decl = _declarations()
    for name in ENTRIES:
        assert name in decl, f"{name} is not declared in include/tgnn.h"
        res, args = decl[name]
        fn = getattr(_lib.lib, name)
        assert [_ctype_of(a) for a in args] == list(fn.argtypes), name
        assert fn.restype is {"int": C.c_int, "size_t": C.c_size_t}[res], name
        assert name in _lib.EXPORTED_SYMBOLS
    # every _many entry takes the layout count first and ends with the stream
    for name in ENTRIES[:4]:
        args = decl[name][1]
        assert args[0] == "int32_t n_layouts" and args[-1] == "tgnn_stream_t stream"


def test_public_functions_have_their_documented_signatures():
    from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver
    from tilingnn_amd.util import algorithms as alg
    sig = inspect.signature(alg.solve_many_by_device_greedy)
    assert list(sig.parameters) == ["ml_solver", "layouts", "seed", "seeds", "score_fn", "max_rounds", "streams"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(seed=0, seeds=None, score_fn=None, max_rounds=100000, streams=3)
    sig = inspect.signature(ML_Solver.solve_many)
    assert list(sig.parameters) == ["self", "brick_layouts", "seed"] and sig.parameters["seed"].default is None
    assert inspect.isclass(alg.PackedLayouts)
    # the single-layout loop keeps its signature
    assert list(inspect.signature(alg.solve_by_device_greedy).parameters) == ["ml_solver", "origin_layout", "seed", "score_fn", "on_round",
                                                                            "max_rounds", "finish"]


def test_arguments_are_checked_before_anything_is_launched():
    from tilingnn_amd import _lib
    lib = _lib.lib
    assert lib.tgnn_sublayout_compact_many_workspace_bytes(-1, 10, 10, 10) == 0
    small, big = (lib.tgnn_sublayout_compact_many_workspace_bytes(k, n, 8 * n, 10 * n) for k, n in ((4, 4000), (189, 200000)))
    assert 0 < small < big < 2 ** 31
    assert 0 < lib.tgnn_greedy_round_many_workspace_bytes(4, 4000) < lib.tgnn_greedy_round_many_workspace_bytes(189, 200000)
    assert lib.tgnn_solution_score_sums_many_workspace_bytes(189) >= 189 * 512 * 3 * 8
    none = [None] * 32
    assert lib.tgnn_sublayout_compact_many(-1, *none[:4], 0, 0, 0, *none[:2], 3, *none[:2], 15, *none[:9], 0, None) == -1
    assert b"number of layouts" in lib.tgnn_last_error()
    assert lib.tgnn_sublayout_compact_many(3, *none[:4], 10, 0, 0, *none[:2], 3, *none[:2], 15, *none[:9], 0, None) == -1
    assert b"offset table" in lib.tgnn_last_error()
    assert lib.tgnn_greedy_round_many(2, *none[:2], 1, *none[:2], 10, 0, *none[:3], 0, *none[:7], 0, None) == -1          # round 0
    assert lib.tgnn_greedy_finish_many(2, *none[:3], 10, 0, *none[:3], 1, 0, *none[:7], None) == -1                        # max_rounds 0
    assert lib.tgnn_solution_score_sums_many(2, *none[:3], 10, 0, *none[:2], 0, *none[:3], 1, *none[:2], 0, None) == -1     # ld_area 0
    # an empty batch is no work and no error
    assert lib.tgnn_sublayout_compact_many(0, *none[:4], 0, 0, 0, *none[:2], 3, *none[:2], 15, *none[:9], 0, None) == 0
