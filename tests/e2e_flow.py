"""End-to-end flow harness: the Dexi+RAFT refinement loop around a correlation block.

Test infrastructure only.  It restates, with functional torch ops, the part of
the reference model that consumes the correlation lookups, so the north-star
criterion "final flow EPE < 1e-3 px (fp32)"  can be checked on
the GPU box without the reference:

  * BasicMotionEncoder / SepConvGRU / FlowHead / mask head
    (reference core/update.py:5-14, 35-60, 81-100, 121-140);
  * the two-volume iteration of RAFT.forward (core/raft.py:165-192): one
    correlation block over (fmap1, fmap2), one over the edge maps
    (fem1, fem2), a shared update block, ``coords1 += delta_flow +
    delta_eflow`` and ``ecoords1 += delta_eflow``;
  * convex 8x upsampling (core/raft.py:87-99).

The encoders (fnet/cnet/efnet/ecnet, DexiNed) are outside the hot path: their
outputs are synthesised by tests/datagen.py (fmaps: the fnet-like distribution;
context: tanh / relu of normals, as core/raft.py:151-158 applies them).
Weights are generated deterministically per reference parameter name (uniform
in +-1/sqrt(fan_in), PyTorch's default Conv2d bound), so the reference model
loaded with the same dict (tests/golden/make_e2e_golden.py) and this harness
compute the same function.
"""
from __future__ import annotations

import zlib

import numpy as np
import torch
import torch.nn.functional as F

import datagen as dg

HDIM = CDIM = 128
RADIUS, LEVELS = 4, 4
CORR_PLANES = LEVELS * (2 * RADIUS + 1) ** 2

# reference BasicUpdateBlock(args(corr_levels=4, corr_radius=4), hidden_dim=128)
# state_dict names and shapes (core/update.py:81-88, 35-44, 6-10, 121-130).
PARAMS = {
    "encoder.convc1": (256, CORR_PLANES, 1, 1),
    "encoder.convc2": (192, 256, 3, 3),
    "encoder.convf1": (128, 2, 7, 7),
    "encoder.convf2": (64, 128, 3, 3),
    "encoder.conv": (126, 256, 3, 3),
    "gru.convz1": (128, 384, 1, 5),
    "gru.convr1": (128, 384, 1, 5),
    "gru.convq1": (128, 384, 1, 5),
    "gru.convz2": (128, 384, 5, 1),
    "gru.convr2": (128, 384, 5, 1),
    "gru.convq2": (128, 384, 5, 1),
    "flow_head.conv1": (256, 128, 3, 3),
    "flow_head.conv2": (2, 256, 3, 3),
    "mask.0": (256, 128, 3, 3),
    "mask.2": (576, 256, 1, 1),
}

# E2E case: config 1 (FlyingChairs 368x496 -> fmap 46x62), 12 iterations.
# ``flow_gain`` scales the flow head's output layer so that random weights give
# displacements of several pixels (taps crossing cells, some off the map).
E2E = {"H": 46, "W": 62, "D": 256, "iters": 12, "weight_seed": 5000, "input_seed": 6000,
       "flow_gain": 8.0}


def update_weights(seed: int = E2E["weight_seed"]) -> dict[str, np.ndarray]:
    """Reference-named state dict (float32 numpy) from the portable generator."""
    out = {}
    for name, shape in PARAMS.items():
        fan_in = shape[1] * shape[2] * shape[3]
        bound = 1.0 / np.sqrt(fan_in)
        if name == "flow_head.conv2":
            bound *= E2E["flow_gain"]
        key = seed + zlib.crc32(name.encode())
        n = int(np.prod(shape))
        out[name + ".weight"] = (bound * (2 * dg.uniform(key, n) - 1)).reshape(shape).astype(np.float32)
        out[name + ".bias"] = (bound * (2 * dg.uniform(key + 1, shape[0]) - 1)).astype(np.float32)
    return out


def e2e_inputs(seed: int = E2E["input_seed"], H: int = E2E["H"], W: int = E2E["W"],
               D: int = E2E["D"]) -> dict[str, np.ndarray]:
    """fmaps (fnet-like) for the image and edge volumes, and context features."""
    out = {k: dg.fmap(seed + i, 1, D, H, W, "fnet") for i, k in enumerate(("fmap1", "fmap2", "fem1", "fem2"))}
    for i, k in enumerate(("net", "inp", "enet", "einp")):
        z = dg.normal(seed + 10 + i, HDIM * H * W).reshape(1, HDIM, H, W)
        z = np.tanh(z) if k in ("net", "enet") else np.maximum(z, 0.0)
        out[k] = z.astype(np.float32)
    return out


def _conv(x, W, name, pad):
    return F.conv2d(x, W[name + ".weight"], W[name + ".bias"], padding=pad)


def sepconv_gru(W, h, x):
    """SepConvGRU.forward (core/update.py:46-60): horizontal then vertical pass."""
    for sfx, pad in (("1", (0, 2)), ("2", (2, 0))):
        hx = torch.cat([h, x], 1)
        z = torch.sigmoid(_conv(hx, W, "gru.convz" + sfx, pad))
        r = torch.sigmoid(_conv(hx, W, "gru.convr" + sfx, pad))
        q = torch.tanh(_conv(torch.cat([r * h, x], 1), W, "gru.convq" + sfx, pad))
        h = (1 - z) * h + z * q
    return h


GRU_NAMES = ("convz1", "convr1", "convq1", "convz2", "convr2", "convq2")


def rne_c(a, cname):
    """float64 tensor -> nearest-even float16 (``"f16"``) or bfloat16 (``"bf16"``),
    as float64; ``None``: the identity.  Rounded straight from the float64 bits, as
    tests/gru_oracle.py::rne does (torch's own double -> 16-bit casts go through
    float32 and round twice).  float16: subnormals kept, 65520 and beyond to +-inf;
    bfloat16: values inside its normal range."""
    assert a.dtype == torch.float64
    if cname is None:
        return a
    drop = {"f16": 42, "bf16": 45}[cname]       # float64 keeps 52 fraction bits, c 10 / 7
    u = a.contiguous().view(torch.int64)        # sign and magnitude: adding rounds |a| up
    u = (u + (((u >> drop) & 1) + ((1 << (drop - 1)) - 1))) & -(1 << drop)
    v = u.view(torch.float64)
    if cname == "f16":
        sub = torch.round(a * 2.0 ** 24) * 2.0 ** -24       # spacing 2^-24 below 2^-14
        v = torch.where(a.abs() < 2.0 ** -14, sub, v)
        v = torch.where(v.abs() >= 65520.0, torch.copysign(torch.full_like(v, float("inf")), a), v)
    return v


def _conv5(a, w, b, axis):
    """b + the zero-padded 5-tap convolution of a [N, C, H, W] with w [Co, C, 5] along
    W (axis 0) or H (axis 1), as five shifted matmuls."""
    N, C, H, Wd = a.shape
    ap = F.pad(a, (2, 2, 0, 0) if axis == 0 else (0, 0, 2, 2))
    P = b[None, :, None, None].expand(N, w.shape[0], H, Wd)
    for t in range(5):
        sl = ap[:, :, :, t:t + Wd] if axis == 0 else ap[:, :, t:t + H, :]
        P = P + torch.einsum("oc,nchw->nohw", w[:, :, t], sl)
    return P


def gru16_emulated(h, x, W, cname):
    """The fused 16-bit GRU's documented roundings (include/dexiraft_gru.h) and nothing
    else, in float64 torch ops on h's device: what tests/gru_oracle.py::forward
    computes in numpy.  Weights, hc = rne_c(h), xc = rne_c(x) and rh = rne_c(r h) are
    rounded to nearest even in c (``cname``: ``"f16"`` / ``"bf16"``; ``None``: no
    rounding); the state between the two passes, the biases, the gates and the blend
    are exact.  ``W`` maps ``[gru.]convz1.weight`` ... ``[gru.]convq2.bias``.  Returns
    float64; no code under test is involved."""
    pre = "gru." if "gru.convz1.weight" in W else ""
    h = torch.as_tensor(h).double()
    xc = rne_c(torch.as_tensor(x).double().to(h.device), cname)
    for axis in range(2):
        w, b = [], []
        for n in GRU_NAMES[3 * axis:3 * axis + 3]:
            wn = torch.as_tensor(W[pre + n + ".weight"]).to(h.device).double()
            w.append(rne_c(wn.reshape(wn.shape[0], wn.shape[1], 5), cname))
            b.append(torch.as_tensor(W[pre + n + ".bias"]).to(h.device).double())
        a = torch.cat([rne_c(h, cname), xc], 1)
        z = torch.sigmoid(_conv5(a, w[0], b[0], axis))
        r = torch.sigmoid(_conv5(a, w[1], b[1], axis))
        q = torch.tanh(_conv5(torch.cat([rne_c(r * h, cname), xc], 1), w[2], b[2], axis))
        h = (1.0 - z) * h + z * q
    return h


def update_block(W, net, inp, corr, flow, gru=None, cor=None, record=None):
    """BasicUpdateBlock.forward (core/update.py:132-140): (net, mask, delta_flow).

    ``gru``: a callable ``(h, x) -> h'`` in place of the float32 SepConvGRU above.
    ``cor``: ``relu(convc1(corr))`` computed by the caller (``corr`` is then unused).
    ``record``: called with ``(net, x)``, the GRU's two arguments, before it runs."""
    # BasicMotionEncoder (core/update.py:90-100)
    if cor is None:
        cor = F.relu(_conv(corr, W, "encoder.convc1", 0))
    cor = F.relu(_conv(cor, W, "encoder.convc2", 1))
    flo = F.relu(_conv(flow, W, "encoder.convf1", 3))
    flo = F.relu(_conv(flo, W, "encoder.convf2", 1))
    out = F.relu(_conv(torch.cat([cor, flo], 1), W, "encoder.conv", 1))
    x = torch.cat([inp, out, flow], 1)
    if record is not None:
        record(net, x)
    h = sepconv_gru(W, net, x) if gru is None else gru(net, x)
    # FlowHead (core/update.py:13-14) and the mask head (core/update.py:126-129,139)
    delta = _conv(F.relu(_conv(h, W, "flow_head.conv1", 1)), W, "flow_head.conv2", 1)
    mask = 0.25 * _conv(F.relu(_conv(h, W, "mask.0", 1)), W, "mask.2", 0)
    return h, mask, delta


def upsample_flow(flow, mask):
    """Convex 8x upsampling (core/raft.py:87-99)."""
    N, _, H, W = flow.shape
    mask = torch.softmax(mask.view(N, 1, 9, 8, 8, H, W), dim=2)
    up = F.unfold(8 * flow, [3, 3], padding=1).view(N, 2, 9, 1, 1, H, W)
    up = torch.sum(mask * up, dim=2).permute(0, 1, 4, 2, 5, 3)
    return up.reshape(N, 2, 8 * H, 8 * W)


def coords_grid(B, H, W, device):
    ys, xs = torch.meshgrid(torch.arange(H, device=device, dtype=torch.float32),
                            torch.arange(W, device=device, dtype=torch.float32), indexing="ij")
    return torch.stack([xs, ys])[None].repeat(B, 1, 1, 1)


def lookup_each(corr_fn, corr_en, coords1, ecoords1, call):
    """The default ``lookup=`` of ``refine``: one call per block, as core/raft.py:172-173."""
    return call(corr_fn, coords1), call(corr_en, ecoords1)


def lookup_batched(corr_both, _, coords1, ecoords1, call):
    """``lookup=`` for one batch-2 block over both volumes:
    ``corr_fn`` is that block (image pair first), ``corr_en`` is unused."""
    return call(corr_both, torch.cat([coords1, ecoords1])).chunk(2)


def refine(corr_fn, corr_en, W, ctx, iters=E2E["iters"], *, gru=None, motion_first=None,
           upsample=None, lookup=None, record=None):
    """RAFT.forward's iteration (core/raft.py:160-192) with given correlation blocks.

    ``corr_fn`` / ``corr_en`` map coords [B,2,H,W] -> [B,324,H,W].  ``ctx`` holds
    net/inp/enet/einp tensors.  Returns (flow_lowres list per iteration,
    final upsampled flow, final edge flow).

    The hooks stand for the substitutions of INTEGRATION.md; each default is the
    reference's own step, so a call without them computes what it always did.
      gru           ``(h, x) -> h'`` in place of the float32 SepConvGRU, both streams
      motion_first  ``(corr_block, coords) -> cor``: lookup + convc1 + ReLU in one
                    call (``CorrBlock.lookup_conv1x1``); its result goes to convc2
      upsample      ``(flow, mask) -> flow_up`` in place of ``upsample_flow``
      lookup        ``(corr_fn, corr_en, coords1, ecoords1, call) -> (image, edge)``:
                    how the blocks are called; ``call(block, coords)`` is
                    ``motion_first`` where given and ``block(coords)`` otherwise
                    (``lookup_each``, the default; ``lookup_batched``; or a function
                    that passes ``out_dtype`` / ``memory_format``).  A 16-bit result
                    is widened to the state's dtype before the update block
      record        ``record(it, stream, net, x, coords, corr)`` once per iteration
                    (from 0) and stream (``"image"``, ``"edge"``), as they occur:
                    the GRU's two arguments, the coordinates looked up and what the
                    lookup (or ``motion_first``) returned for them
    """
    net, inp, enet, einp = ctx["net"], ctx["inp"], ctx["enet"], ctx["einp"]
    B, _, H, Wd = net.shape
    coords0 = coords_grid(B, H, Wd, net.device)
    coords1 = coords0.clone()
    ecoords0 = coords_grid(B, H, Wd, net.device)
    ecoords1 = ecoords0.clone()
    lookup = lookup or lookup_each
    upsample = upsample or upsample_flow
    call = motion_first or (lambda block, coords: block(coords))
    flows = []
    up = None
    for it in range(iters):
        corr, ecorr = lookup(corr_fn, corr_en, coords1, ecoords1, call)
        flow = coords1 - coords0
        eflow = ecoords1 - ecoords0
        steps = []
        for stream, h, ctx_in, c, fl, cds in (("image", net, inp, corr, flow, coords1),
                                              ("edge", enet, einp, ecorr, eflow, ecoords1)):
            rec = None
            if record is not None:
                rec = (lambda n, x, s=stream, c=c, cds=cds: record(it, s, n, x, cds, c))
            c = c.to(h.dtype)
            steps.append(update_block(W, h, ctx_in, None if motion_first else c, fl, gru=gru,
                                      cor=c if motion_first else None, record=rec))
        (net, up_mask, delta_flow), (enet, _, delta_eflow) = steps
        coords1 = coords1 + delta_flow + delta_eflow
        ecoords1 = ecoords1 + delta_eflow
        flows.append(coords1 - coords0)
        up = upsample(coords1 - coords0, up_mask)
    return flows, up, ecoords1 - ecoords0


def epe(a, b) -> float:
    """Mean end-point error (px) between two flow fields [B,2,H,W]."""
    a = torch.as_tensor(a, dtype=torch.float64).cpu()
    b = torch.as_tensor(b, dtype=torch.float64).cpu()
    return float(torch.sqrt(((a - b) ** 2).sum(1)).mean())


def torch_weights(W: dict[str, np.ndarray], device) -> dict[str, torch.Tensor]:
    return {k: torch.from_numpy(v).to(device) for k, v in W.items()}


class E2EModel:
    """A ``model(image1, image2, iters=, test_mode=True) -> (flow_low, flow_up)``
    for ``driver.infer_pairs`` (the reference RAFT.forward signature,
    core/raft.py:101): the refinement loop above around ``block_cls`` blocks.
    The encoders are out of scope, so the "images" only select the synthetic
    encoder outputs: pair p is an image whose pixels all equal p, and its
    inputs are ``e2e_inputs(E2E['input_seed'] + 97 * p)`` (p = 0: the golden's)."""

    def __init__(self, block_cls, device, weights=None):
        self.block_cls = block_cls
        self.device = device
        self.W = torch_weights(weights or update_weights(), device)

    def inputs(self, p: int) -> dict[str, torch.Tensor]:
        x = e2e_inputs(E2E["input_seed"] + 97 * p)
        return {k: torch.from_numpy(v).to(self.device) for k, v in x.items()}

    def __call__(self, image1, image2, iters=E2E["iters"], test_mode=True):
        p = int(round(float(image1.reshape(-1)[0])))
        t = self.inputs(p)
        corr_fn = self.block_cls(t["fmap1"], t["fmap2"])
        corr_en = self.block_cls(t["fem1"], t["fem2"])
        flows, up, _ = refine(corr_fn, corr_en, self.W, t, iters)
        return flows[-1], up
