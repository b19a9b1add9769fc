"""A/B of the 32- and 64-pixel gate tiles of the fused SepConvGRU.

Builds csrc/gru_sepconv.hip twice, with DXG_TILE64_ABOVE_WGS set so that every
gate launch takes the 32-pixel form (tile32) or, for lines longer than 32 pixels,
the 64-pixel form (tile64), into optical-flow_dexi-raft_amd/build/ab/, loads both
beside the package's own library and times dxg_sepconv_gru of each: same process,
interleaved rounds, captured graphs of 12 calls, each arm twice (A/A).  bfloat16,
Ch = 128, Cx = 256.  One JSON line per shape, appended to --out.

Usage: python scripts/ab_gru_tiles.py [--build-only] [--out FILE]
"""
import argparse
import ctypes
import importlib.util
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
PKG = REPO / "optical-flow_dexi-raft_amd"
AB_DIR = PKG / "build" / "ab"
VARIANTS = {"tile32": 2_000_000_000, "tile64": 0}

ap = argparse.ArgumentParser()
ap.add_argument("--build-only", action="store_true")
ap.add_argument("--out", default=str(REPO / "profiles" / "r22" / "gru" / "ab_tiles_bfloat16.jsonl"))
args = ap.parse_args()

spec = importlib.util.spec_from_file_location("_dxr_build", PKG / "build.py")
bld = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bld)
bld.build()
AB_DIR.mkdir(parents=True, exist_ok=True)
for name, above in VARIANTS.items():
    so = AB_DIR / f"libgru_{name}.so"
    src = PKG / "csrc" / "gru_sepconv.hip"
    if not so.exists() or so.stat().st_mtime < src.stat().st_mtime:
        subprocess.run([bld.hipcc(), *bld.CXXFLAGS, f"-DDXG_TILE64_ABOVE_WGS={above}", "-shared",
                        "-o", str(so), str(src), f"-L{PKG}", f"-l:{bld.LIB_NAME}",
                        "-Wl,-rpath,$ORIGIN/../.."], check=True)
if args.build_only:
    raise SystemExit(0)

sys.path.insert(0, str(REPO))
import dexiraft_amd  # noqa: E402,F401
from dexiraft_amd import _native  # noqa: E402

_native.load()
LIBS = {}
for name in VARIANTS:
    lib = ctypes.CDLL(str(AB_DIR / f"libgru_{name}.so"))
    for fn, (res, argt) in _native.GRU_SIGNATURES.items():
        getattr(lib, fn).restype = res
        getattr(lib, fn).argtypes = argt
    LIBS[name] = lib
ARMS = ["tile32", "tile64", "tile32_again", "tile64_again"]
SHAPES = {"sintel_b1": (1, 55, 128), "sintel_b2": (2, 55, 128), "sintel_b4": (4, 55, 128),
          "chairs_b6": (6, 46, 62), "chairs_b2": (2, 46, 62)}
CH, CX = 128, 256
dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev)
gen.manual_seed(22)
K = 5 * (CH + CX)
BF = _native.DXG_BF16
F32 = _native.DXG_F32
out_path = Path(args.out)
out_path.parent.mkdir(parents=True, exist_ok=True)
results = []
with torch.no_grad():
    w = []
    for i in range(6):
        shape = (CH, CH + CX, 1, 5) if i < 3 else (CH, CH + CX, 5, 1)
        w.append((torch.randn(shape, generator=gen, device=dev) / K ** 0.5,
                  0.5 * torch.randn(CH, generator=gen, device=dev)))
    lib0 = LIBS["tile32"]
    nb = lib0.dxg_sepconv_packed_weight_bytes(CH, CX)
    packed = []
    s0 = torch.cuda.current_stream(dev).cuda_stream
    for axis in range(2):
        t = w[3 * axis:3 * axis + 3]
        buf = torch.empty(nb, dtype=torch.uint8, device=dev)
        st = lib0.dxg_sepconv_pack_weights(t[0][0].data_ptr(), t[1][0].data_ptr(), t[2][0].data_ptr(),
                                           t[0][1].data_ptr(), t[1][1].data_ptr(), t[2][1].data_ptr(),
                                           CH, CX, BF, buf.data_ptr(), nb, s0)
        assert st == 0, st
        packed.append(buf)
    torch.cuda.synchronize()
    for shape, (N, H, W) in SHAPES.items():
        h = torch.tanh(torch.randn((N, CH, H, W), generator=gen, device=dev))
        x = torch.randn((N, CX, H, W), generator=gen, device=dev)
        wsb = lib0.dxg_sepconv_workspace_bytes(N, H, W, CH, CX)
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))

        def call(lib, out, ws):
            st = lib.dxg_sepconv_gru(h.data_ptr(), F32, x.data_ptr(), F32, packed[0].data_ptr(),
                                     packed[1].data_ptr(), N, H, W, CH, CX, BF, out.data_ptr(), F32,
                                     ws.data_ptr(), wsb, torch.cuda.current_stream(dev).cuda_stream)
            assert st == 0, st

        with torch.cuda.stream(stream):
            graphs, outs = {}, {}
            for name, lib in LIBS.items():
                out = torch.empty_like(h)
                ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
                call(lib, out, ws)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=stream):
                    for _ in range(12):
                        call(lib, out, ws)
                graphs[name], outs[name] = g, (out, ws)
            stream.synchronize()
            same = bool(torch.equal(outs["tile32"][0], outs["tile64"][0]))
            t_end = time.perf_counter() + 0.5
            while time.perf_counter() < t_end:
                for g in graphs.values():
                    g.replay()
                stream.synchronize()
            us = {a: [] for a in ARMS}
            for _ in range(11):
                for a in ARMS:
                    g = graphs[a.split("_")[0]]
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(5):
                        g.replay()
                    e1.record(stream)
                    stream.synchronize()
                    us[a].append(e0.elapsed_time(e1) * 1e3 / 60)
        torch.cuda.current_stream(dev).wait_stream(stream)
        rec = {"shape": shape, "N": N, "H": H, "W": W, "compute_dtype": "bfloat16",
               "tiles32_h": N * H * ((W + 31) // 32), "tiles32_v": N * W * ((H + 31) // 32),
               "outputs_equal": same,
               "us_per_call": {a: {"median": statistics.median(v), "min": min(v), "max": max(v)}
                               for a, v in us.items()}}
        results.append(rec)
        print(json.dumps(rec), flush=True)
        with out_path.open("a") as f:
            f.write(json.dumps(rec) + "\n")
