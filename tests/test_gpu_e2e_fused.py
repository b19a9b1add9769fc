"""GPU: the 12-iteration refinement loop (tests/e2e_flow.py, golden
tests/golden/e2e_chairs.npz: 46x62, D = 256, r = 4, 4 levels, final flows beyond 8 px)
with INTEGRATION.md's inference substitutions in it, alone and together, on one
stream, one allocator pool and in one captured graph.

  a  ``lookup_conv1x1`` (§6), the batch-2 block (§5), channels-last lookups (§7) and
     ``upsample_flow``: the float32 criteria of tests/test_e2e_flow.py, and at every
     iteration the substituted call against the plain one on the same coordinates.
  b  ``SepConvGRU`` in the loop.  d is the EPE against the golden of the same loop
     around ``e2e_flow.gru16_emulated`` (float64 torch ops with the documented
     roundings; tests/test_e2e_fused_cpu.py holds it to tests/gru_oracle.py), so it
     is what the operand rounding alone costs; the module's loop stays within 2 d,
     the factor and reason of test_gpu_gru.py::test_end_to_end_against_the_reference.
  c  one ``SepConvGRU`` call on (net, x) as the loop produces them, and aliasing.
  d  the mixed-precision path: float16 fmaps, float16 pyramid, float16 lookups.
  e  everything of a and the bfloat16 GRU in one captured graph.

tests/test_e2e_fused_cpu.py shows on the host that each criterion used here fails
for a wrong piece.
"""
from __future__ import annotations

import contextlib
import copy
from functools import lru_cache

import numpy as np
import pytest
import torch

import e2e_flow as ef
import e2e_fused as fu

pytestmark = pytest.mark.gpu

EPE_F32 = 1e-3      # px, the fp32 criterion of tests/test_e2e_flow.py
CNAME = {torch.float16: "f16", torch.bfloat16: "bf16"}
DTYPES = [torch.float16, torch.bfloat16]
FMAPS = ("fmap1", "fmap2", "fem1", "fem2")


def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda", 0)


@contextlib.contextmanager
def deterministic_convolutions():
    """For the tests that compare two runs of the loop bit for bit: have torch pick
    deterministic convolution algorithms for the update block while they run."""
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = old


def inputs(p: int = 0) -> dict:
    x = ef.e2e_inputs(ef.E2E["input_seed"] + 97 * p)
    return {k: torch.from_numpy(v).to(dev()) for k, v in x.items()}


class Setup:
    """Built once per module and read only: the golden's inputs, the weights, the two
    float32 blocks, and the plain float32 loop with its states at iterations 1, 6, 12."""

    def __init__(self):
        import dexiraft_amd as dx
        self.dx = dx
        self.W = ef.torch_weights(ef.update_weights(), dev())
        self.t = inputs()
        self.conv = (self.W["encoder.convc1.weight"], self.W["encoder.convc1.bias"])
        self.gru_weights = {k[4:]: v for k, v in self.W.items() if k.startswith("gru.")}
        with torch.no_grad():
            self.fn = dx.CorrBlock(self.t["fmap1"], self.t["fmap2"])
            self.en = dx.CorrBlock(self.t["fem1"], self.t["fem2"])
            self.states = fu.States([1, 6, 12])
            self.f32 = fu.quantities(*ef.refine(self.fn, self.en, self.W, self.t, record=self.states))
        fu.show("float32 loop", self.f32)
        fu.assert_f32_class(self.f32, EPE_F32)

    def ref_lookup(self, stream, coords):
        return (self.fn if stream == "image" else self.en)(coords)

    def ref_fused(self, stream, coords):
        return (self.fn if stream == "image" else self.en).lookup_conv1x1(coords, *self.conv)

    def both(self, t=None):
        t = t or self.t
        return self.dx.CorrBlock(torch.cat([t["fmap1"], t["fem1"]]), torch.cat([t["fmap2"], t["fem2"]]))

    def run(self, fn=None, en=None, **hooks):
        with torch.no_grad():
            return ef.refine(fn or self.fn, en or self.en, self.W, self.t, **hooks)


@lru_cache(maxsize=None)
def setup() -> Setup:
    return Setup()


# ----------------------------------------------------- a. float32-class substitutions
def _cl_lookup(fn, en, coords1, ecoords1, call):
    return (fn(coords1, memory_format=torch.channels_last),
            en(ecoords1, memory_format=torch.channels_last))


@pytest.mark.parametrize("which", ["lookup_conv1x1", "batched", "channels_last", "upsample", "all"])
def test_float32_substitutions(which):
    s = setup()
    dx, (w, b) = s.dx, s.conv
    ups = []

    def upsample(flow, mask):
        ups.append(tuple(mask.shape))
        return dx.upsample_flow(flow, mask)

    if which == "lookup_conv1x1":
        hooks = dict(motion_first=lambda blk, c: blk.lookup_conv1x1(c, w, b))
        check = fu.LookupCheck(s.ref_lookup, conv=s.conv)
    elif which == "batched":
        hooks = dict(fn=s.both(), lookup=ef.lookup_batched)
        check = fu.LookupCheck(s.ref_lookup)
    elif which == "channels_last":
        hooks = dict(lookup=_cl_lookup)
        check = fu.LookupCheck(s.ref_lookup, channels_last=True)
    elif which == "upsample":
        hooks, check = dict(upsample=upsample), fu.LookupCheck(s.ref_lookup)
    else:
        # the fused call on the batch-2 block, stored channels-last: each half equals the
        # fused call on its own block (NCHW) as values, and is within 1e-6 of float64
        hooks = dict(fn=s.both(), lookup=ef.lookup_batched, upsample=upsample,
                     motion_first=lambda blk, c: blk.lookup_conv1x1(
                         c, w, b, memory_format=torch.channels_last))
        check = fu.LookupCheck(s.ref_lookup, conv=s.conv, ref_fused=s.ref_fused, channels_last=True)
    flows, up, eflow = s.run(record=check, **hooks)
    q = fu.quantities(flows, up, eflow)
    fu.show(which, q)
    if check.conv is not None:
        print(f"lookup_conv1x1 in the loop: {check.worst:.2e} of max against float64")
    assert check.calls == 2 * ef.E2E["iters"]
    if "upsample" in hooks:
        assert ups == [(1, 576, ef.E2E["H"], ef.E2E["W"])] * ef.E2E["iters"]
    assert up.shape == (1, 2, 8 * ef.E2E["H"], 8 * ef.E2E["W"]) and up.dtype == torch.float32
    fu.assert_f32_class(q, EPE_F32)


# ------------------------------------------------------------ b. the 16-bit GRU, looped
@pytest.mark.parametrize("c", DTYPES, ids=["f16", "bf16"])
def test_fused_gru_in_the_loop(c):
    """Measured on an MI355X (px; d: the emulated loop against the golden, i.e. the
    documented operand rounding alone; then the module's loop against the golden):

                 final      upsampled  edge flow   of 2 d used   module vs emulated (final)
      d_f16      2.854e-03  1.610e-02  1.708e-03
      module     2.855e-03  1.610e-02  1.708e-03   0.500         1.2e-04
      d_bf16     2.512e-02  1.574e-01  1.386e-02
      module     2.513e-02  1.574e-01  1.387e-02   0.500         8.0e-04

    The largest per-iteration value is the final one in all four loops.  d_bf16 is
    above EPE_BF16 = 1e-2 px of tests/test_e2e_flow.py: on this loop the
    documented bfloat16 operand rounding alone, before any kernel, costs 2.5e-2 px;
    float16 stays below it ("Update block").  The float32 loop itself
    is at 5.6e-06 px.  The last digit moves from run to run: torch's float32
    convolutions of the update block are not run-to-run deterministic here.
    """
    s = setup()
    cn = CNAME[c]
    emulated = s.run(gru=lambda h, x: ef.gru16_emulated(h, x, s.W, cn).float())
    d = fu.quantities(*emulated)
    fu.show(f"d_{cn}: emulated loop against the golden", d)
    fu.assert_rounding_in_play(d, s.f32)

    mod = s.dx.SepConvGRU(s.gru_weights, compute_dtype=c)
    got = s.run(gru=mod)
    q = fu.quantities(*got)
    fu.show(f"SepConvGRU {cn} loop against the golden", q)
    print(f"SepConvGRU {cn} loop against the emulated loop: final {ef.epe(got[0][-1], emulated[0][-1]):.3e} px, "
          f"upsampled {ef.epe(got[1], emulated[1]):.3e}, edge {ef.epe(got[2], emulated[2]):.3e}")
    fu.assert_within(f"SepConvGRU {cn} loop", q, d)


# ------------------------------------------- c. one fused call on states as they occur
@pytest.mark.parametrize("c", DTYPES, ids=["f16", "bf16"])
def test_fused_gru_on_states_of_the_loop(c):
    """(net, x) of the image stream at iterations 1, 6 and 12 of the float32 loop:
    reference-named weights with ``flow_gain``, states after many updates, real
    motion features.  The rule of test_end_to_end_against_the_reference: the module
    is within 2 d of the float32 torch GRU, d the distance of the float64 definition
    with the roundings (``gru16_emulated``: gru_oracle.forward to 1e-12, at these
    channel counts too, tests/test_e2e_fused_cpu.py) from the same."""
    s = setup()
    cn = CNAME[c]
    mod = s.dx.SepConvGRU(s.gru_weights, compute_dtype=c)
    assert sorted(s.states.kept) == [1, 6, 12]
    for it, (net, x) in sorted(s.states.kept.items()):
        with torch.no_grad():
            ref = ef.sepconv_gru(s.W, net, x).double()
            d = float((ef.gru16_emulated(net, x, s.W, cn) - ref).abs().max())
            h0, x0 = net.clone(), x.clone()
            out = mod(net, x)
        err = float((out.double() - ref).abs().max())
        print(f"iteration {it} {cn}: d = {d:.3e}, module vs float32 GRU {err:.3e} ({err / d:.2f} d)")
        assert out.dtype == torch.float32 and np.isfinite(err) and err <= 2 * d
        # aliasing: the inputs are left as they were; h = mod(h, x) twice in a row is
        # the same two calls on clones
        assert torch.equal(net, h0) and torch.equal(x, x0)
        assert out.data_ptr() != net.data_ptr()
        with torch.no_grad():
            h = net
            h = mod(h, x)
            h = mod(h, x)
            want = mod(mod(h0.clone(), x0.clone()).clone(), x0.clone())
        torch.cuda.synchronize()
        assert torch.equal(h, want)


# ---------------------------------------------------------- d. the mixed-precision path
def _cast_block(dx, f1, f2):
    """The plain block with torch casts: the float32 block of the widened fmaps, its
    pyramid levels replaced by ``level.half()`` (widened again, packed back by
    ``dxr_pyramid_pack``; float32 kernels, not under test here)."""
    from dexiraft_amd import _native as nat
    lib = nat.load()
    cb = dx.CorrBlock(f1.float(), f2.float())
    B, D, H, W = cb._geom
    buf = torch.zeros(cb._buf.numel(), dtype=torch.float32, device=cb._buf.device)
    for lvl, lev in enumerate(cb.corr_pyramid):
        lev = lev.half().float().contiguous()
        assert lib.dxr_pyramid_pack(lev.data_ptr(), B, H, W, cb.num_levels, lvl, buf.data_ptr(),
                                    nat.DXR_F32, nat.stream_of(buf)) == nat.DXR_OK
    torch.cuda.synchronize()
    ref = copy.copy(cb)
    ref._buf, ref._ref_pyramid = buf, None
    return ref


@lru_cache(maxsize=None)
def mixed():
    s = setup()
    f = {k: s.t[k].half() for k in FMAPS}
    with torch.no_grad():
        blocks = {"image": s.dx.CorrBlock(f["fmap1"], f["fmap2"], pyramid_dtype=torch.float16),
                  "edge": s.dx.CorrBlock(f["fem1"], f["fem2"], pyramid_dtype=torch.float16)}
        casts = {"image": _cast_block(s.dx, f["fmap1"], f["fmap2"]),
                 "edge": _cast_block(s.dx, f["fem1"], f["fem2"])}
    return f, blocks, casts


@pytest.mark.parametrize("fused", [False, True], ids=["lookup", "lookup_conv1x1"])
def test_mixed_precision_path(fused):
    """float16 fmaps, ``pyramid_dtype=torch.float16`` and float16 lookup outputs (once
    the plain lookup, once ``lookup_conv1x1``) against the plain loop with torch casts
    at the same places: fmaps ``.half().float()``, pyramid levels ``.half()``, the
    lookup (or lookup + convc1 + ReLU) ``.half()``.  Every lookup equals the cast one
    bit for bit.  Measured on an MI355X (px, against the golden):

                               final      upsampled  edge flow   of 2 d used
      lookup          d        1.009e-03  2.639e-03  7.228e-04
                      loop     1.007e-03  2.633e-03  7.223e-04   0.500
      lookup_conv1x1  d        9.917e-04  2.532e-03  7.084e-04
                      loop     9.908e-04  2.535e-03  7.089e-04   0.501

    With equal lookups the two loops would be equal too; they differ in the last
    digits because torch's float32 convolutions of the update block are not
    run-to-run deterministic here, which the margin of 2 d covers with room.
    """
    s = setup()
    w, b = s.conv
    _, blocks, casts = mixed()
    assert blocks["image"]._buf.dtype == torch.float16
    h16 = torch.float16
    if fused:
        hooks = dict(motion_first=lambda blk, c: blk.lookup_conv1x1(c, w, b, out_dtype=h16))
        cast_hooks = dict(motion_first=lambda blk, c: blk.lookup_conv1x1(c, w, b).half())
        check = fu.LookupCheck(lambda st, c: casts[st](c), conv=s.conv, cast=h16,
                               ref_fused=lambda st, c: casts[st].lookup_conv1x1(c, w, b))
    else:
        hooks = dict(lookup=lambda fn, en, c, ec, call: (fn(c, out_dtype=h16), en(ec, out_dtype=h16)))
        cast_hooks = dict(lookup=lambda fn, en, c, ec, call: (fn(c).half(), en(ec).half()))
        check = fu.LookupCheck(lambda st, c: casts[st](c), cast=h16)
    d = fu.quantities(*s.run(casts["image"], casts["edge"], **cast_hooks))
    fu.show("d: the float32 loop with torch casts", d)
    fu.assert_rounding_in_play(d, s.f32)
    got = s.run(blocks["image"], blocks["edge"], record=check, **hooks)
    assert check.calls == 2 * ef.E2E["iters"]
    q = fu.quantities(*got)
    fu.show("mixed-precision loop", q)
    fu.assert_within("mixed-precision loop", q, d)


def test_alternate_block_on_float16_fmaps():
    """``AlternateCorrBlock`` reads float16 fmaps in place; its contract is value
    equality with the block on the widened fmaps, so the two loops' flows are equal."""
    s = setup()
    f, _, _ = mixed()
    alt = s.dx.AlternateCorrBlock
    with torch.no_grad(), deterministic_convolutions():
        wide = {"image": alt(f["fmap1"].float(), f["fmap2"].float()),
                "edge": alt(f["fem1"].float(), f["fem2"].float())}
        check = fu.LookupCheck(lambda st, c: wide[st](c))      # every lookup, bit for bit
        a = s.run(alt(f["fmap1"], f["fmap2"]), alt(f["fem1"], f["fem2"]), record=check)
        b = s.run(wide["image"], wide["edge"])
    assert check.calls == 2 * ef.E2E["iters"] and len(a[0]) == ef.E2E["iters"]
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(x, y), f"iteration {i + 1}"
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    fu.show("AlternateCorrBlock on float16 fmaps", fu.quantities(*a))


# ------------------------------------------------------- e. everything in one graph
def test_whole_loop_in_one_graph():
    """The substitutions of a and the bfloat16 GRU, the block construction included,
    captured on one side stream after an eager warm-up there (weights packed and
    convolution algorithms chosen outside the capture): the replay equals eager on
    the golden's inputs, on another pair's inputs copied into the static tensors, and
    on two further replays.  Both volumes live in the one batch-2 block of §5."""
    s = setup()
    dx, (w, b) = s.dx, s.conv
    mod = dx.SepConvGRU(s.gru_weights, compute_dtype=torch.bfloat16)
    static = {k: v.clone() for k, v in s.t.items()}
    other = inputs(1)

    def loop(t):
        flows, up, eflow = ef.refine(
            s.both(t), None, s.W, t, gru=mod, lookup=ef.lookup_batched, upsample=dx.upsample_flow,
            motion_first=lambda blk, c: blk.lookup_conv1x1(c, w, b, memory_format=torch.channels_last))
        return flows + [up, eflow]

    def same(a, b):
        return len(a) == len(b) == ef.E2E["iters"] + 2 and all(torch.equal(x, y) for x, y in zip(a, b))

    stream = torch.cuda.Stream(device=dev())
    stream.wait_stream(torch.cuda.current_stream(dev()))
    with torch.no_grad(), deterministic_convolutions(), torch.cuda.stream(stream):
        eager = [x.clone() for x in loop(static)]
        eager_other = [x.clone() for x in loop(other)]
        assert not same(eager, eager_other)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = loop(static)
        for x in out:
            x.zero_()
        graph.replay()
        stream.synchronize()
        assert same(out, eager)
        fu.show("graph replay (bfloat16 GRU, everything fused)", fu.quantities(out[:-2], out[-2], out[-1]))
        for k, v in other.items():              # another pair through the same graph
            static[k].copy_(v)
        graph.replay()
        stream.synchronize()
        assert same(out, eager_other)
        for _ in range(2):
            graph.replay()
            stream.synchronize()
            assert same(out, eager_other)
    torch.cuda.current_stream(dev()).wait_stream(stream)
