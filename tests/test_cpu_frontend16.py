"""CPU tier of the text frontend's 16-bit mode: the surface (header, binding, library, Python switch, the command line),
the end-to-end gate held by CPU realisations of the spec alone (tests/frontend16_oracle.py), and the sharpness of both
gates against injected defects.  The GPU tier (tests/test_gpu_frontend16.py) holds the device to the same gates."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import frontend16_oracle as f16o
from tests import frontend_oracle as fo
from wetts_amd import _lib, frontend, frontend_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="needs a built wetts_amd/lib/libwetts_hip.so")
CASES = [(c, lens) for c in fo.CONFIGS for lens in fo.FIXTURE_SHAPES]
NEW = ("wetts_frontend_set_precision", "wetts_frontend_get_precision", "wetts_frontend_linear16_workspace_bytes",
       "wetts_frontend_linear16", "wetts_frontend_linear16_form")


# ---- 1. surface ------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_new_entries_and_the_abi_version_stays():
    header = open(os.path.join(ROOT, "include", "wetts_hip.h"), encoding="utf-8").read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"#define\s+WETTS_ABI_VERSION\s+12\b", header) and _lib.ABI_VERSION == 12
    assert len(_lib.SIGNATURES["wetts_frontend_linear16"][1]) == 14
    assert "frontend16.hip" in __import__("wetts_amd.build", fromlist=["SOURCES"]).SOURCES


@needs_lib
def test_library_exports_the_entries_and_refuses_bad_arguments_before_any_launch():
    """Every refusal below returns WETTS_E_INVALID from host checks alone: this test runs without a device."""
    lib = _lib.load()
    assert lib.wetts_abi_version() == 12
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.wetts_frontend_set_precision(None, 1) == -1 and "null" in _lib.last_error()
    assert lib.wetts_frontend_get_precision(None) < 0
    fake = C.create_string_buffer(4096)  # never read: the precision is checked before the handle is touched
    for bad in (-1, 3, 16):
        assert lib.wetts_frontend_set_precision(C.cast(fake, C.c_void_p), bad) == -1 and "precision" in _lib.last_error()
    assert lib.wetts_frontend_linear16_workspace_bytes(312, 936) == 312 * 936 * 2
    assert lib.wetts_frontend_linear16_workspace_bytes(12, 8) < 0 and lib.wetts_frontend_linear16_workspace_bytes(8, 6) < 0
    N, K, M = 3, 16, 8
    x, w, b, r, y = torch.zeros(N, K), torch.zeros(M, K), torch.zeros(M), torch.zeros(N, M), torch.full((N, M), 7.0)
    ws = torch.zeros(K * M // 2 + 4)

    def call(x=x, w=w, b=b, r=r, N=N, K=K, M=M, epi=0, prec=1, form=0, y=y, ws=ws, nbytes=K * M * 2):
        return lib.wetts_frontend_linear16(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(r), N, K, M, epi, prec, form,
                                           _lib.ptr(y), _lib.ptr(ws), nbytes, None)

    for kw, word in ((dict(K=12), "multiple of 8"), (dict(K=0), "multiple of 8"), (dict(M=6), "multiple of 8"),
                     (dict(epi=4), "epilogue"), (dict(epi=-1), "epilogue"), (dict(epi=3, r=None), "epilogue"),
                     (dict(prec=0), "precision"), (dict(prec=3), "precision"), (dict(form=4), "form"), (dict(form=-1), "form"), (dict(form=16 | 4), "form"),
                     (dict(N=0), "bad argument"), (dict(x=None), "bad argument"), (dict(w=None), "bad argument"),
                     (dict(y=None), "bad argument"), (dict(ws=None), "workspace"), (dict(nbytes=K * M * 2 - 1), "workspace"),
                     # every operand moves in 16-byte pieces: one float off is refused, the residual only where it is read
                     (dict(x=torch.zeros(N * K + 1)[1:]), "aligned"), (dict(w=torch.zeros(M * K + 1)[1:]), "aligned"),
                     (dict(b=torch.zeros(M + 1)[1:]), "aligned"), (dict(epi=3, r=torch.zeros(N * M + 1)[1:]), "aligned"),
                     (dict(y=torch.zeros(N * M + 1)[1:]), "aligned"), (dict(ws=ws[1:]), "aligned")):
        assert call(**kw) == -1, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    assert bool((y == 7.0).all())
    # the launcher's choice, as form 0 takes it: the K split up to 64 tokens; beyond them the 128-token tile where
    # ceil(M / 128) ceil(N / 128) >= 512 (M = 1024: from 63 x 128 + 1 tokens) and the 64-token tile below
    for n, m, form in ((1, 4, 1), (64, 3072, 1), (65, 36, 2), (65, 3072, 2), (63 * 128, 1024, 2), (63 * 128 + 1, 1024, 3),
                       (4096, 768, 2), (4096, 2304, 3), (4096, 3072, 3)):
        assert lib.wetts_frontend_linear16_form(n, m) == form, (n, m)
    assert lib.wetts_frontend_linear16_form(0, 8) < 0 and lib.wetts_frontend_linear16_form(8, 6) < 0


def test_set_dtype_before_to_is_remembered_and_bad_names_are_refused():
    m = frontend.FrontendModel(fo.NUM_POLYPHONES, fo.NUM_PROSODY, fo.BERT_CONFIGS["tiny"])
    assert m._precision == 0 and m.dtype == torch.float32
    for name, prec, dt in ((torch.bfloat16, 1, torch.bfloat16), ("bf16", 1, torch.bfloat16), (torch.float16, 2, torch.float16),
                           ("fp16", 2, torch.float16), ("f16", 2, torch.float16), (torch.float32, 0, torch.float32),
                           ("f32", 0, torch.float32), ("fp32", 0, torch.float32)):
        assert m.set_dtype(name) is m and m._precision == prec and m.dtype == dt, name
    for bad in (torch.float64, "int8", torch.uint8, 1):
        with pytest.raises(ValueError, match="dtype"):
            m.set_dtype(bad)
    assert m._precision == 0
    assert frontend.frontend_precision(None) == 0
    with pytest.raises(ValueError, match="dtype"):
        frontend.Frontend("/nonexistent", dtype="int4")  # refused before any file is read
    import inspect
    for fn in (frontend.load_frontend_model, frontend.Frontend.__init__, frontend.FrontendSession.__init__):
        p = inspect.signature(fn).parameters
        assert "dtype" in p and p["dtype"].default is None, fn


def test_frontend_eval_parses_dtype():
    base = ["--polyphone_dict", "a", "--prosody_dict", "b", "--checkpoint", "c"]
    for cmd, extra in (("cv", ["--cv_polyphone_data", "x", "--cv_prosody_data", "y"]), ("polyphone", ["--test_data", "x"]),
                       ("prosody", ["--test_data", "x"])):
        assert frontend_eval.get_args([cmd] + base + extra).dtype == "f32"
        for t in ("f32", "bf16", "f16"):
            assert frontend_eval.get_args([cmd] + base + extra + ["--dtype", t]).dtype == t
        with pytest.raises(SystemExit):
            frontend_eval.get_args([cmd] + base + extra + ["--dtype", "int8"])


# ---- 2. the end-to-end gate holds for the spec alone -------------------------------------------------------------------------
@pytest.mark.parametrize("tname", list(f16o.DTYPES))
@pytest.mark.parametrize("cname,lens", CASES)
def test_float32_realisations_stay_within_three_d_of_the_float64_model(cname, lens, tname):
    """Both float32 realisations of the spec (torch's summation order; K in 8 interleaved chunks added pairwise), every
    output, both measures: within 3 x D of frontend_oracle.forward(float64 weights)."""
    D, ids, mask, st64 = f16o.precision_loss(cname, lens, tname)
    for k in fo.OUTPUTS:
        assert D[k][0] > 10 * fo.HALF_ULP, (k, D[k])  # the mode loses precision: D is not a rounding artefact
    W32 = fo.weights(cname)[0]
    for linear in (f16o.linear16, f16o.linear16_split8):
        got = f16o.forward16(W32, cname, ids, mask, f16o.DTYPES[tname], linear=linear)
        mult = f16o.e2e_multiples(got, st64, mask, D)
        print(fo.case_name(cname, lens), tname, linear.__name__, {k: tuple(round(x, 3) for x in v) for k, v in mult.items()})
        assert f16o.e2e_worst(mult) <= f16o.E2E_FACTOR, (linear.__name__, mult)
        for k in fo.OUTPUTS:
            assert not bool(got[k][mask == 0].any()), k


# ---- 3. sharpness ------------------------------------------------------------------------------------------------------------
SHARP_CASES = (("base", (33, 32, 31)), ("tiny", (9, 6)))


@pytest.mark.parametrize("tname", list(f16o.DTYPES))
@pytest.mark.parametrize("cname,lens", SHARP_CASES)
def test_injected_model_defects_fail_the_end_to_end_gate(cname, lens, tname):
    """no_position, swap_qk, no_residual, softmax_axis, pad_key and transform_12_heads (a defect only where the config's
    transform has another head count: the base branch) land outside 3 x D.  tanh_gelu and eps_1e-5 are NOT expected to be
    seen end to end: they lie inside the mode's own precision loss (they are seen at f32, tests/test_cpu_frontend.py)."""
    D, ids, mask, st64 = f16o.precision_loss(cname, lens, tname)
    W32 = fo.weights(cname)[0]
    for fault in f16o.SEEN_FAULTS:
        if fault == "transform_12_heads" and fo.config(cname)["transform_heads"] == 12:
            continue
        got = f16o.forward16(W32, cname, ids, mask, f16o.DTYPES[tname], fault=fault)
        worst = f16o.e2e_worst(f16o.e2e_multiples(got, st64, mask, D))
        print(cname, tname, fault, round(worst, 2))
        assert worst > f16o.E2E_FACTOR, (fault, worst)


def _truncate(t, dtype):
    """Round toward zero to the type (the defect: the low bits dropped instead of round to nearest even)."""
    keep = 16 if dtype == torch.bfloat16 else 13
    bits = t.contiguous().view(torch.int32) & ~((1 << keep) - 1)
    return bits.view(torch.float32)


@pytest.mark.parametrize("tname", list(f16o.DTYPES))
@pytest.mark.parametrize("K", (312, 768))
def test_injected_launch_defects_fail_the_per_launch_gate_and_clean_realisations_pass(K, tname):
    """x left unrounded, W left unrounded, truncation instead of RNE, a dropped last K step, the K % 16 == 8 tail read as
    garbage: each fails gate 1 or gate 2; torch's float32 evaluation and the 8-chunk one pass both."""
    dtype = f16o.DTYPES[tname]
    N, M = 37, 100
    x, w, b, res = f16o.random_launch(N, K, M, 16000 + K)
    xq, wq = f16o.q(x, dtype), f16o.q(w, dtype)
    for epi in range(4):
        r = res if epi == 3 else None

        def finish(y):
            return f16o._epilogue(y + r if epi == 3 else y, epi)

        for linear in (F.linear, f16o.split8):
            m = f16o.launch_multiples(f16o.linear_f32(x, w, b, r, dtype, epi, linear), x, w, b, r, dtype, epi)
            assert f16o.launch_ok(m), (epi, linear.__name__, m)
        garbage = torch.full((N, 8), 3.0), torch.full((M, 8), 0.25)
        defects = {
            "x_unrounded": finish(F.linear(x, wq, b)),
            "w_unrounded": finish(F.linear(xq, w, b)),
            "truncation": finish(F.linear(_truncate(x, dtype), _truncate(w, dtype), b)),
            "dropped_last_k_step": finish(F.linear(xq[:, :K - 16], wq[:, :K - 16], b)),
        }
        if K % 16 == 8:
            defects["garbage_tail"] = finish(F.linear(torch.cat([xq, garbage[0]], 1), torch.cat([wq, garbage[1]], 1), b))
        for name, got in defects.items():
            m = f16o.launch_multiples(got, x, w, b, r, dtype, epi)
            print(K, tname, epi, name, m)
            assert not f16o.launch_ok(m), (epi, name, m)
