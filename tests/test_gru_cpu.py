"""CPU: the SepConvGRU C-ABI (include/dexiraft_gru.h, prefix dxg_, in
libdexiraft_gru.so) beside the untouched export list of libdexiraft_corr.so, its
host-side validation (every refusal returns before any launch, so these calls are
safe without a GPU), the byte-size functions, the CPU-side refusals of
``dexiraft_amd.SepConvGRU``, and the float64 oracle the GPU tests compare against
(tests/gru_oracle.py), pinned to outputs of the reference's own SepConvGRU."""
from __future__ import annotations

import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import gru_oracle as go
from conftest import GOLDEN, REPO

HEADER = REPO / "include" / "dexiraft_gru.h"
DXG = {"dxg_abi_version", "dxg_sepconv_packed_weight_bytes", "dxg_sepconv_pack_weights",
       "dxg_sepconv_workspace_bytes", "dxg_sepconv_pack_inputs", "dxg_sepconv_gate_zr",
       "dxg_sepconv_gate_qh", "dxg_sepconv_gru"}
GOLDENS = ("gru_c16_b2", "gru_c32")


def declared(header, prefix: str) -> set[str]:
    pat = re.compile(r"^\s*(?:int|int64_t|const char\*)\s+(" + prefix + r"\w+)\s*\(", re.M)
    return set(pat.findall(header.read_text()))


def exported(path) -> set[str]:
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True,
                         check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


@pytest.fixture(scope="module")
def nat():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "_dxr_build_t", REPO / "optical-flow_dexi-raft_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()  # no-op when fresh
    from dexiraft_amd import _native
    _native.load_gru()
    return _native


def load_golden(name):
    with np.load(GOLDEN / f"{name}.npz") as z:
        seed, N, H, W, Ch, Cx = (int(v) for v in z["case"])
        out, checksum = z["out"], z["input_checksum"]
    h, x, weights = go.case(seed, N, H, W, Ch, Cx)
    np.testing.assert_allclose([h.astype(np.float64).sum(), x.astype(np.float64).sum()], checksum,
                               rtol=0, atol=1e-6)
    return h, x, weights, out


@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_without_roundings_reproduces_the_reference(name):
    """Every rne_c the identity: the oracle is the reference's float32 forward to
    1e-5 of its largest output.  Pins the tap order, the gate order and the padding
    (the weights differ in every tap and channel)."""
    h, x, weights, out = load_golden(name)
    got = go.forward(h, x, weights, None)
    assert got.shape == out.shape
    err = np.abs(got - out).max() / np.abs(out).max()
    print(f"{name}: oracle vs reference {err:.2e} of max")
    assert err <= 1e-5


def test_oracle_roundings():
    """rne: float16 as numpy's, bfloat16 as torch's, ties to even in both.  A check of
    the oracle itself (test infrastructure): it needs no part of the library."""
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.normal(0, 1, 4000), rng.normal(0, 1e-3, 1000), [0.0, -0.0, 1.0],
                        1 + 2.0 ** -8 * np.arange(1, 8, 2),      # bfloat16 ties
                        1 + 2.0 ** -11 * np.arange(1, 8, 2)]).astype(np.float32)
    t = torch.from_numpy(a)
    assert np.array_equal(go.rne(a, "bf16"), t.bfloat16().double().numpy())
    assert np.array_equal(go.rne(a, "f16"), t.half().double().numpy())
    assert go.rne(a, None).dtype == np.float64 and np.array_equal(go.rne(a, None), a)
    big = a[np.abs(a) >= 2.0 ** -14].astype(np.float64)    # float16's normal range
    for c, p in go.P_BITS.items():
        assert (np.abs(go.rne(big, c) - big) <= 2.0 ** -p * np.abs(big)).all()


def test_header_declares_exactly_the_gru_entry_points():
    assert declared(HEADER, "dxg_") == DXG
    for other in ("dxr_", "dxf_", "dxu_", "dxl_"):
        assert declared(HEADER, other) == set()
    text = HEADER.read_text()
    assert re.search(r"^#define DXG_ABI_VERSION 1$", text, re.M)
    for lines in ("core/update.py:45-60", "core/update.py:47-49", "core/update.py:50-51",
                  "core/update.py:36-42"):
        assert lines in text                              # the reference lines it replaces
    for name in ("DXG_F32", "DXG_F16", "DXG_BF16"):
        assert name in text


def test_library_exports_the_gru_symbols(nat):
    syms = exported(nat.GRU_LIB_PATH)
    assert {s for s in syms if s.startswith("dx")} == DXG == set(nat.GRU_SIGNATURES)
    # the correlation library's export list has no part of it
    assert not {s for s in exported(nat.LIB_PATH) if s.startswith("dxg_")}
    lib = nat.load_gru()
    for name in DXG:
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
    assert lib.dxg_abi_version() == nat.GRU_ABI_VERSION == 1
    assert (nat.DXG_F32, nat.DXG_F16, nat.DXG_BF16) == (0, 1, 2)


BAD_GEOMETRY = ((-1, 8, 8, 16, 32), (1, 0, 8, 16, 32), (1, 8, 0, 16, 32), (1, -8, -8, 16, 32),
                (1, 8, 8, 0, 32), (1, 8, 8, 16, 0), (1, 8, 8, -16, 32), (1, 8, 8, 16, -32))
UNSUPPORTED = ((1, 8, 8, 8, 32), (1, 8, 8, 24, 32), (1, 8, 8, 144, 32), (1, 8, 8, 16, 8),
               (1, 8, 8, 16, 40), (1, 8, 8, 16, 272), (1, 8, 8, 96, 1 << 40),
               (65536, 8, 8, 16, 32), (1, 2048, 2049, 16, 32), (1, 1 << 22, 2, 16, 32),
               (1, 1 << 40, 1 << 40, 16, 32), (1, 1 << 62, 4, 16, 32))


def test_host_side_validation_needs_no_gpu(nat):
    lib = nat.load_gru()
    P = 1 << 12   # a non-null, 16-byte aligned dummy address: never dereferenced on these paths
    OK, EINVAL, EUNSUP = nat.DXR_OK, nat.DXR_EINVAL, nat.DXR_EUNSUPPORTED
    F32, F16, BF16 = nat.DXG_F32, nat.DXG_F16, nat.DXG_BF16
    BIG = 1 << 60
    pw, pi = lib.dxg_sepconv_pack_weights, lib.dxg_sepconv_pack_inputs
    zr, qh, gru = lib.dxg_sepconv_gate_zr, lib.dxg_sepconv_gate_qh, lib.dxg_sepconv_gru

    # the four calls that take (N, H, W, Ch, Cx), each with otherwise good arguments
    def calls(geo, c=F16, ws=P, nbytes=BIG):
        return {"pack_inputs": pi(P, F32, P, F32, *geo, c, ws, nbytes, None),
                "gate_zr": zr(P, 0, *geo, c, ws, nbytes, None),
                "gate_qh": qh(P, 1, *geo, c, P, F32, ws, nbytes, None),
                "gate_qh_state": qh(P, 0, *geo, c, None, F32, ws, nbytes, None),
                "gru": gru(P, F32, P, F32, P, P, *geo, c, P, F32, ws, nbytes, None)}

    good = (2, 5, 7, 16, 32)
    need = lib.dxg_sepconv_workspace_bytes(*good)
    assert need == 2 * 5 * 7 * (12 * 16 + 2 * 32)
    # N == 0 is OK before anything else is looked at
    assert pi(None, 99, None, 99, 0, -1, -1, 7, 7, 99, None, 0, None) == OK
    assert zr(None, 9, 0, -1, -1, 7, 7, 99, None, 0, None) == OK
    assert qh(None, 9, 0, -1, -1, 7, 7, 99, None, 99, None, 0, None) == OK
    assert gru(None, 99, None, 99, None, None, 0, -1, -1, 7, 7, 99, None, 99, None, 0, None) == OK
    for geo in BAD_GEOMETRY[1:]:
        assert set(calls(geo).values()) == {EINVAL}, geo
    assert set(calls(BAD_GEOMETRY[0]).values()) == {EINVAL}
    for geo in UNSUPPORTED:
        assert set(calls(geo).values()) == {EUNSUP}, geo
    for c in (F32, -1, 3, 0x100):
        assert set(calls(good, c=c).values()) == {EINVAL}, c          # compute dtype
    for ws, nbytes in ((None, BIG), (P + 8, BIG), (P, need - 1), (P, 0), (P, -1)):
        assert set(calls(good, ws=ws, nbytes=nbytes).values()) == {EINVAL}, (ws, nbytes)
    for c in (F16, BF16):
        for dt in (-1, 3, 0x100):
            assert pi(P, dt, P, F32, *good, c, P, need, None) == EINVAL   # h / x / out dtypes
            assert pi(P, F32, P, dt, *good, c, P, need, None) == EINVAL
            assert qh(P, 1, *good, c, P, dt, P, need, None) == EINVAL
            assert gru(P, dt, P, F32, P, P, *good, c, P, F32, P, need, None) == EINVAL
            assert gru(P, F32, P, dt, P, P, *good, c, P, F32, P, need, None) == EINVAL
            assert gru(P, F32, P, F32, P, P, *good, c, P, dt, P, need, None) == EINVAL
        assert pi(None, F32, P, F32, *good, c, P, need, None) == EINVAL   # null pointers
        assert pi(P, F32, None, F32, *good, c, P, need, None) == EINVAL
        for axis in (-1, 2, 7):
            assert zr(P, axis, *good, c, P, need, None) == EINVAL
            assert qh(P, axis, *good, c, P, F32, P, need, None) == EINVAL
        for packed in (None, P + 4):
            assert zr(packed, 0, *good, c, P, need, None) == EINVAL
            assert qh(packed, 0, *good, c, None, F32, P, need, None) == EINVAL
            assert gru(P, F32, P, F32, packed, P, *good, c, P, F32, P, need, None) == EINVAL
            assert gru(P, F32, P, F32, P, packed, *good, c, P, F32, P, need, None) == EINVAL
        assert gru(None, F32, P, F32, P, P, *good, c, P, F32, P, need, None) == EINVAL
        assert gru(P, F32, None, F32, P, P, *good, c, P, F32, P, need, None) == EINVAL
        assert gru(P, F32, P, F32, P, P, *good, c, None, F32, P, need, None) == EINVAL
    # pack_weights: (wz, wr, wq, bz, br, bq, Ch, Cx, compute_dtype, packed, packed_bytes, stream)
    pb = lib.dxg_sepconv_packed_weight_bytes(16, 32)
    six = [P] * 6
    for ch, cx in ((0, 32), (16, 0), (-16, 32)):
        assert pw(*six, ch, cx, F16, P, BIG, None) == EINVAL
    for geo in UNSUPPORTED[:7]:
        assert pw(*six, *geo[3:], F16, P, BIG, None) == EUNSUP, geo
    for c in (F32, -1, 3):
        assert pw(*six, 16, 32, c, P, pb, None) == EINVAL
    for k in range(6):
        args = list(six)
        args[k] = None
        assert pw(*args, 16, 32, BF16, P, pb, None) == EINVAL
    for packed, nbytes in ((None, pb), (P + 8, pb), (P, pb - 1), (P, 0)):
        assert pw(*six, 16, 32, BF16, packed, nbytes, None) == EINVAL
    assert nat.load().dxr_last_hip_error() == 0


def test_byte_size_functions(nat):
    """-1 for bad or unsupported geometry, multiples of 16, room for what the header
    says they hold, and non-decreasing in every argument."""
    lib = nat.load_gru()
    wb, pb = lib.dxg_sepconv_workspace_bytes, lib.dxg_sepconv_packed_weight_bytes
    for bad in BAD_GEOMETRY + UNSUPPORTED:
        assert wb(*bad) == -1, bad
    assert wb(0, 8, 8, 16, 32) == 0
    assert wb(65535, 2048, 2048, 128, 256) == 65535 * (1 << 22) * (12 * 128 + 2 * 256)
    for n, h, w, ch, cx in ((1, 1, 1, 16, 16), (2, 5, 67, 16, 32), (1, 55, 128, 128, 256),
                            (6, 46, 62, 96, 64)):
        b = wb(n, h, w, ch, cx)
        assert b % 16 == 0 and b == n * h * w * (12 * ch + 2 * cx)
    by_w = [wb(1, 1, n, 16, 32) for n in range(1, 3000)]
    assert by_w == sorted(by_w) and by_w == [wb(1, n, 1, 16, 32) for n in range(1, 3000)]
    by_n = [wb(n, 55, 127, 128, 256) for n in (0, 1, 2, 3, 7, 8, 64, 1024, 65535)]
    assert by_n == sorted(by_n)
    chans = range(16, 129, 16), range(16, 257, 16)
    by_ch = [wb(2, 9, 11, ch, 32) for ch in chans[0]]
    by_cx = [wb(2, 9, 11, 64, cx) for cx in chans[1]]
    assert by_ch == sorted(by_ch) and by_cx == sorted(by_cx)
    for ch, cx in ((0, 32), (16, 0), (-16, 32), (8, 32), (24, 32), (144, 32), (16, 8), (16, 272)):
        assert pb(ch, cx) == -1, (ch, cx)
    for ch in chans[0]:
        for cx in chans[1]:
            b, rows = pb(ch, cx), 2 * ch + (ch + 31) // 32 * 32
            # rows x K 16-bit weights and rows float32 biases
            assert b % 16 == 0 and 0 <= b - (10 * (ch + cx) + 4) * rows < 16
    assert [pb(ch, 32) for ch in chans[0]] == sorted(pb(ch, 32) for ch in chans[0])
    assert [pb(64, cx) for cx in chans[1]] == sorted(pb(64, cx) for cx in chans[1])


def test_python_shell_refusals():
    import dexiraft_amd as dx
    from dexiraft_amd import gru as gru_mod
    assert dx.SepConvGRU is gru_mod.SepConvGRU and "SepConvGRU" in dx.__all__
    _, _, weights, _ = load_golden("gru_c16_b2")
    weights = {k: torch.from_numpy(v) for k, v in weights.items()}
    g = dx.SepConvGRU(weights, compute_dtype=torch.float16)
    assert (g.hidden_dim, g.input_dim, g.compute_dtype) == (16, 32, torch.float16)
    assert dx.SepConvGRU(weights).compute_dtype == torch.bfloat16
    h, x = torch.zeros(2, 16, 5, 7), torch.zeros(2, 32, 5, 7)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="HIP device"):
            g(h, x)                                                   # host tensors
        with pytest.raises(RuntimeError, match="HIP device"):
            g(h.half(), x.bfloat16())
    # grad mode on and something requires grad: refused, and before any device work
    with pytest.raises(RuntimeError, match="inference"):
        g(h.clone().requires_grad_(), x)
    with pytest.raises(RuntimeError, match="inference"):
        g(h, x.clone().requires_grad_())

    class Conv:
        def __init__(self, w, b):
            self.weight, self.bias = w, b

    class Module:
        pass

    m = Module()
    for n in go.NAMES:
        setattr(m, n, Conv(weights[f"{n}.weight"].clone().requires_grad_(), weights[f"{n}.bias"]))
    gm = dx.SepConvGRU.from_module(m, compute_dtype=torch.bfloat16)
    assert (gm.hidden_dim, gm.input_dim) == (16, 32)
    with pytest.raises(RuntimeError, match="inference"):
        gm(h, x)                                                      # a weight requires grad
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP device"):
        gm(h, x)
    with pytest.raises(ValueError, match="convq2"):
        delattr(m, "convq2")
        dx.SepConvGRU.from_module(m)
    # shapes, dtypes
    with torch.no_grad():
        for hh, xx in ((h[0], x), (h, x[0]), (h[:, :8], x), (h, x[:, :16]), (h[:1], x),
                       (h[:, :, :4], x), (h, x[..., :6]), (x, h)):
            with pytest.raises(ValueError):
                g(hh, xx)
        with pytest.raises(ValueError):
            g(h, x.to("meta"))                                        # different devices
        for dt in (torch.float64, torch.int32):
            with pytest.raises(TypeError):
                g(h.to(dt), x)
            with pytest.raises(TypeError):
                g(h, x.to(dt))
        with pytest.raises(TypeError):
            g(h.numpy(), x)
    # construction: compute dtype, unsupported channels, wrong shapes
    for dt in (torch.float32, torch.float64):
        with pytest.raises(ValueError, match="compute_dtype"):
            dx.SepConvGRU(weights, compute_dtype=dt)

    def made(ch, cx):
        w = {}
        for i, n in enumerate(go.NAMES):
            w[f"{n}.weight"] = torch.zeros((ch, ch + cx, 1, 5) if i < 3 else (ch, ch + cx, 5, 1))
            w[f"{n}.bias"] = torch.zeros(ch)
        return w

    for ch, cx in ((8, 32), (24, 32), (144, 32), (16, 8), (16, 40), (16, 272), (96, 64 + 8)):
        with pytest.raises(ValueError, match="unsupported channels"):
            dx.SepConvGRU(made(ch, cx))
    assert dx.SepConvGRU(made(128, 256)).hidden_dim == 128
    bad = made(16, 32)
    bad["convr2.weight"] = torch.zeros(16, 48, 1, 5)                  # a horizontal shape
    with pytest.raises(ValueError, match="convr2"):
        dx.SepConvGRU(bad)
    bad = made(16, 32)
    del bad["convq1.bias"]
    with pytest.raises(ValueError):
        dx.SepConvGRU(bad)
