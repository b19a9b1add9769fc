"""dexiraft_amd — MI355X-native RAFT correlation subsystem (Dexi+RAFT hot path).

Import name ``dexiraft_amd`` (see ``dexiraft_amd.py`` at the repository root,
which maps it onto this ``optical-flow_dexi-raft_amd/`` directory).

Public surface, mirroring the reference's interface for this path:
  * ``CorrBlock``, ``AlternateCorrBlock``  — core/corr.py:12-91
  * ``TrainableAlternateCorrBlock``        — the on-the-fly block with fmap gradients
  * ``alt_cuda_corr.forward / backward``  — alt_cuda_corr/correlation.cpp:51-54
  * ``coords_grid``                        — core/utils/utils.py:74-77
  * ``forward_interpolate``                — core/utils/utils.py:26-54, on the GPU
  * ``upsample_flow``                      — core/raft.py:87-98, fused, with its backward
  * ``sequence_loss``                      — train.py:48-73, fused, with its backward
  * ``SepConvGRU``                         — core/update.py:33-60, the inference forward
    on the matrix cores (float16 / bfloat16 operands, float32 state)
  * ``flow_metrics``                       — the EPE reductions of evaluate.py, on the GPU
  * ``driver.InputPadder / write_flo / infer_pairs`` — core/utils/utils.py:7-24,
    core/utils/frame_utils.py:70-99, evaluate.py's per-pair loop (sharded)
  * ``driver.infer_sequence``              — evaluate.py:33-50, the warm-started sequence
"""
from . import alt_cuda_corr, driver
from ._native import LIB_PATH, load as load_native
from .corr import AlternateCorrBlock, CorrBlock, TrainableAlternateCorrBlock
from .gru import SepConvGRU
from .utils import coords_grid, flow_metrics, forward_interpolate, sequence_loss, upsample_flow

__all__ = ["CorrBlock", "AlternateCorrBlock", "TrainableAlternateCorrBlock", "alt_cuda_corr", "coords_grid", "forward_interpolate", "upsample_flow", "sequence_loss", "flow_metrics", "SepConvGRU", "driver",
           "load_native", "LIB_PATH"]
__version__ = "0.1.0"
