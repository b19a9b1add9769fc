"""What keeps tests/test_gpu_e2e_fused.py honest, checked where no kernel runs.

  * ``e2e_flow.gru16_emulated`` (the float64 torch restatement of the fused GRU's
    documented roundings, the source of the GPU tests' margin d) equals
    tests/gru_oracle.py::forward.
  * ``e2e_flow.refine`` with every hook left at its default returns the tensors the
    loop returned before it had hooks (a copy of that code is kept below).
  * The hooks are live, and the GPU tests' criteria (tests/e2e_fused.py) can fail:
    around plain restatements of the fused pieces (the numpy oracle's block, torch's
    conv + ReLU, the emulated GRU) they pass, and with a GRU that skips the vertical
    pass, a lookup + convc1 without the ReLU, or a batched block whose two
    coordinate sets are swapped, every criterion that covers the piece fails.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import e2e_flow as ef
import e2e_fused as fu
import gru_oracle as go
from test_e2e_flow import EPE_F32, EPE_HARNESS, _OracleBlock

SHORT = 2       # iterations of the loops below: a wrong hook shows in the first one


@pytest.mark.parametrize("cname", ["f16", "bf16"])
@pytest.mark.parametrize("shape", [(2, 5, 67, 16, 32), (1, 3, 70, 128, 256)],
                         ids=["2x5x67_c16", "1x3x70_c128"])
def test_gru16_emulated_equals_the_oracle(shape, cname):
    """Both are float64 sums of the same rounded operands in different orders, on
    values of order one: 1e-12 absolute."""
    h, x, weights = go.case(9300 + shape[2], *shape)
    want = go.forward(h, x, weights, cname)
    got = ef.gru16_emulated(torch.from_numpy(h), torch.from_numpy(x), weights, cname)
    assert got.dtype == torch.float64 and tuple(got.shape) == want.shape
    err = float(np.abs(got.numpy() - want).max())
    print(f"{shape} {cname}: max |emulated - oracle| = {err:.2e}")
    assert err <= 1e-12
    # the rounding is there: without it the result moves by far more than that
    exact = ef.gru16_emulated(torch.from_numpy(h), torch.from_numpy(x), weights, None)
    assert float(np.abs(exact.numpy() - want).max()) > 1e-5


def test_rne_c_equals_the_oracles_rounding():
    """Ties both ways, float16's subnormal range and its overflow, and values that
    a cast through float32 would round twice."""
    rng = np.random.default_rng(7)
    v = np.concatenate([rng.standard_normal(50000) * s for s in (1.0, 1e-4, 1e-6, 3e4)])
    edge = [65519.9, 65520.0, -65520.0, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25,
            1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -40, -1 - 2.0 ** -8,
            1 + 2.0 ** -8 + 2.0 ** -40, 0.0, -0.0]
    v = np.concatenate([v, edge])
    for cname in ("f16", "bf16"):
        a = v if cname == "f16" else v[np.abs(v) > 1e-30]
        assert np.array_equal(ef.rne_c(torch.from_numpy(a), cname).numpy(), go.rne(a, cname)), cname
    twice = torch.tensor([1 + 2.0 ** -11 + 2.0 ** -40], dtype=torch.float64)
    assert ef.rne_c(twice, "f16").item() == 1 + 2.0 ** -10 and twice.float().half().item() == 1.0


# ------------------------------------------------- the loop as it was before the hooks
def _old_update_block(W, net, inp, corr, flow):
    _conv = ef._conv
    cor = F.relu(_conv(corr, W, "encoder.convc1", 0))
    cor = F.relu(_conv(cor, W, "encoder.convc2", 1))
    flo = F.relu(_conv(flow, W, "encoder.convf1", 3))
    flo = F.relu(_conv(flo, W, "encoder.convf2", 1))
    out = F.relu(_conv(torch.cat([cor, flo], 1), W, "encoder.conv", 1))
    x = torch.cat([inp, out, flow], 1)
    h = net
    for sfx, pad in (("1", (0, 2)), ("2", (2, 0))):
        hx = torch.cat([h, x], 1)
        z = torch.sigmoid(_conv(hx, W, "gru.convz" + sfx, pad))
        r = torch.sigmoid(_conv(hx, W, "gru.convr" + sfx, pad))
        q = torch.tanh(_conv(torch.cat([r * h, x], 1), W, "gru.convq" + sfx, pad))
        h = (1 - z) * h + z * q
    delta = _conv(F.relu(_conv(h, W, "flow_head.conv1", 1)), W, "flow_head.conv2", 1)
    mask = 0.25 * _conv(F.relu(_conv(h, W, "mask.0", 1)), W, "mask.2", 0)
    return h, mask, delta


def _old_refine(corr_fn, corr_en, W, ctx, iters):
    net, inp, enet, einp = ctx["net"], ctx["inp"], ctx["enet"], ctx["einp"]
    B, _, H, Wd = net.shape
    coords0 = ef.coords_grid(B, H, Wd, net.device)
    coords1 = coords0.clone()
    ecoords0 = ef.coords_grid(B, H, Wd, net.device)
    ecoords1 = ecoords0.clone()
    flows = []
    up = None
    for _ in range(iters):
        corr = corr_fn(coords1)
        ecorr = corr_en(ecoords1)
        flow = coords1 - coords0
        eflow = ecoords1 - ecoords0
        net, up_mask, delta_flow = _old_update_block(W, net, inp, corr, flow)
        enet, _, delta_eflow = _old_update_block(W, enet, einp, ecorr, eflow)
        coords1 = coords1 + delta_flow + delta_eflow
        ecoords1 = ecoords1 + delta_eflow
        flows.append(coords1 - coords0)
        up = ef.upsample_flow(coords1 - coords0, up_mask)
    return flows, up, ecoords1 - ecoords0


class _Setup:
    """The golden's inputs on the host, the oracle's two blocks and their batch-2 form."""

    def __init__(self):
        torch.set_num_threads(8)
        x = ef.e2e_inputs()
        self.W = ef.torch_weights(ef.update_weights(), "cpu")
        self.t = {k: torch.from_numpy(v) for k, v in x.items()}
        t = self.t
        self.fn = _OracleBlock(t["fmap1"], t["fmap2"])
        self.en = _OracleBlock(t["fem1"], t["fem2"])
        self.both = _OracleBlock(torch.cat([t["fmap1"], t["fem1"]]), torch.cat([t["fmap2"], t["fem2"]]))
        self.conv = (self.W["encoder.convc1.weight"], self.W["encoder.convc1.bias"])

    def ref_lookup(self, stream, coords):
        return (self.fn if stream == "image" else self.en)(coords)

    def motion(self, relu=True):
        w, b = self.conv

        def first(block, coords):
            y = F.conv2d(block(coords), w, b)
            return F.relu(y) if relu else y
        return first

    def run(self, iters=SHORT, fn=None, **hooks):
        with torch.no_grad():
            return ef.refine(fn or self.fn, self.en, self.W, self.t, iters, **hooks)


@pytest.fixture(scope="module")
def s():
    return _Setup()


def test_default_hooks_change_nothing(s):
    iters = 3
    with torch.no_grad():
        old = _old_refine(s.fn, s.en, s.W, s.t, iters)
    new = s.run(iters)
    assert len(new[0]) == len(old[0]) == iters
    for a, b in zip(new[0], old[0]):
        assert torch.equal(a, b)
    assert torch.equal(new[1], old[1]) and torch.equal(new[2], old[2])
    fu.assert_f32_class(fu.quantities(new[0]), EPE_HARNESS)
    # the hooks named explicitly are the same loop, and record= sees every step once
    seen = []
    named = s.run(iters, gru=lambda h, x: ef.sepconv_gru(s.W, h, x), upsample=ef.upsample_flow,
                  lookup=ef.lookup_each,
                  record=lambda it, stream, net, x, coords, corr: seen.append((it, stream, tuple(x.shape))))
    assert all(torch.equal(a, b) for a, b in zip(named[0], old[0])) and torch.equal(named[1], old[1])
    assert seen == [(i, st, (1, 256, ef.E2E["H"], ef.E2E["W"])) for i in range(iters)
                    for st in ("image", "edge")]


def test_float32_class_substitutions_pass_and_wrong_ones_fail(s):
    """Criteria a (and d's equality) around plain pieces: conv + ReLU after the
    oracle's lookup for ``lookup_conv1x1``, the oracle's batch-2 block for §5."""
    check = fu.LookupCheck(s.ref_lookup, conv=s.conv)
    flows, _, _ = s.run(motion_first=s.motion(), record=check)
    fu.assert_f32_class(fu.quantities(flows), EPE_F32)
    assert check.calls == 2 * SHORT and check.worst <= fu.CONV1X1_OF_MAX
    check = fu.LookupCheck(s.ref_lookup)
    flows, _, _ = s.run(fn=s.both, lookup=ef.lookup_batched, record=check)
    fu.assert_f32_class(fu.quantities(flows), EPE_F32)
    assert check.calls == 2 * SHORT

    # lookup + convc1 without the ReLU: the in-loop check, the flow criterion, and the
    # 16-bit equality of d each fail
    with pytest.raises(AssertionError, match="iteration 1"):
        s.run(motion_first=s.motion(relu=False), record=fu.LookupCheck(s.ref_lookup, conv=s.conv))
    q = fu.quantities(s.run(motion_first=s.motion(relu=False))[0])
    fu.show("no ReLU", q)
    with pytest.raises(AssertionError):
        fu.assert_f32_class(q, EPE_F32)
    half = lambda f: (lambda block, coords: f(block, coords).half())     # noqa: E731
    cast = dict(conv=s.conv, cast=torch.float16,
                ref_fused=lambda stream, coords: s.motion()(s.fn if stream == "image" else s.en, coords))
    s.run(motion_first=half(s.motion()), record=fu.LookupCheck(s.ref_lookup, **cast))
    with pytest.raises(AssertionError, match="iteration 1"):
        s.run(motion_first=half(s.motion(relu=False)), record=fu.LookupCheck(s.ref_lookup, **cast))

    # the batched block's coordinate sets swapped.  The two streams start from the same
    # grid, so the first lookups agree and the check fails from the second iteration on
    def swapped(both, _, coords1, ecoords1, call):
        return call(both, torch.cat([ecoords1, coords1])).chunk(2)
    with pytest.raises(AssertionError, match="iteration 2, image stream"):
        s.run(fn=s.both, lookup=swapped, record=fu.LookupCheck(s.ref_lookup))
    q = fu.quantities(s.run(fn=s.both, lookup=swapped)[0])
    fu.show("swapped coordinates", q)
    with pytest.raises(AssertionError):
        fu.assert_f32_class(q, EPE_F32)


@pytest.mark.parametrize("cname", ["f16", "bf16"])
def test_gru_margin_passes_the_emulation_and_fails_a_gru_without_its_vertical_pass(s, cname):
    """Criteria b and c.  d comes from the emulated GRU.  A GRU with the same roundings
    and float32 sums (the fused kernel's arithmetic class: here torch's float32
    convolutions on the rounded operands) stays within 2 d; one that returns the
    state after the horizontal pass does not, in the loop or on one call."""
    W = s.W

    def emulated(h, x):
        return ef.gru16_emulated(h, x, W, cname).float()

    def rounded_f32(h, x, passes=2):
        r = lambda a: ef.rne_c(a.double(), cname).float()       # noqa: E731
        Wc = {k: (r(v) if k.endswith("weight") else v) for k, v in W.items() if k.startswith("gru.")}
        xc = r(x)
        for sfx, pad in (("1", (0, 2)), ("2", (2, 0)))[:passes]:
            hx = torch.cat([r(h), xc], 1)
            z = torch.sigmoid(ef._conv(hx, Wc, "gru.convz" + sfx, pad))
            g = torch.sigmoid(ef._conv(hx, Wc, "gru.convr" + sfx, pad))
            q = torch.tanh(ef._conv(torch.cat([r(g * h), xc], 1), Wc, "gru.convq" + sfx, pad))
            h = (1 - z) * h + z * q
        return h

    states = fu.States([SHORT])
    f32 = fu.quantities(s.run(record=states)[0])
    d = fu.quantities(s.run(gru=emulated)[0])
    fu.show(f"emulated {cname} loop (d)", d)
    fu.assert_rounding_in_play(d, f32)
    fu.assert_within(f"{cname} float32-sum GRU", fu.quantities(s.run(gru=rounded_f32)[0]), d)
    bad = fu.quantities(s.run(gru=lambda h, x: rounded_f32(h, x, passes=1))[0])
    fu.show("no vertical pass", bad)
    with pytest.raises(AssertionError):
        fu.assert_within("no vertical pass", bad, d)
    # c: one call on a state as it occurs
    net, x = states.kept[SHORT]
    ref = ef.sepconv_gru(W, net, x).double()
    dd = float((ef.gru16_emulated(net, x, W, cname) - ref).abs().max())
    ok = float((rounded_f32(net, x).double() - ref).abs().max())
    wrong = float((rounded_f32(net, x, passes=1).double() - ref).abs().max())
    print(f"one call {cname}: d = {dd:.3e}, float32-sum GRU {ok:.3e}, no vertical pass {wrong:.3e}")
    assert ok <= 2 * dd < wrong
