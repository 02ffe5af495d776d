"""diffusiondepth_amd -- MI355X-native DDIM denoise hot path of DiffusionDepth.

Host side (this package, Python because the reference is Python) mirrors the reference's
head / pipeline / scheduler / depth-transform interfaces; all arithmetic on the hot path runs in
``libddepth_hip.so`` (hand-written HIP for gfx950, C ABI in ``include/ddepth.h``).  There is no CPU
fallback: importing works anywhere, running needs the built library and a GPU.
"""
import os as _os

# The HIP 7.0 runtime's graph fast path ("packet capture") corrupts long runs of hipGraph replays next to eager launches (profiles/r06_experiments.md section 10);
# the runtime reads this switch ONCE, at its first HIP call.  GRAPH_REPLAY_SAFE = the process's environment ALREADY had it = 0 when this package was imported (the
# job exported it; bench.py, the tests and the entry points set it in their first lines): only then do this binding's handles replay their loops as hipGraphs.
# Otherwise the variable is exported here for what it is worth (it takes effect if no HIP call has happened yet -- which this package cannot know: even
# torch.cuda.is_available() initialises the runtime) and the handles enqueue their loops EAGERLY: the same kernels in the same order, measured at the same rate.
GRAPH_REPLAY_SAFE = _os.environ.get("DEBUG_CLR_GRAPH_PACKET_CAPTURE") == "0"
_os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

from .scheduler import DDIMScheduler
from .backend import HipDenoiser, precision_id, library_path, load_library
from .modules import ScheduledCNNRefine, CNNDDIMPipiline, DeepDepthTransformWithUpsampling
from .head import (DDIMDepthEstimate_Res, DDIMDepthEstimate_Swin_ADD, DDIMDepthEstimate_Swin_ADDHAHI, DDIMDepthEstimate_MPVIT_ADDHAHI,
                   DDIMDepthEstimate_ResVis, DDIMDepthEstimate_Swin_ADDHAHIVis)
from .necks import HAHIHeteroNeck
from .nlspn import NLSPN
from .model import Diffusion_DCbase_Model, fuse_basic_block_tails, fuse_conv_bn_stats
from .metric import Diffusion_DCbase_Metric, MetricAccumulator
from .loss import Diffusion_DCbase_Loss
from .batchnorm import HipBatchNorm2d, convert_hip_batchnorm
from .conv import HipConv2d, HipConvTranspose2d, convert_hip_conv, conv_bn_train
from .codec import HipCodecConv2d, HipCodecConvTranspose2d, HipCodecTail, convert_hip_codec
from .swin import (HipShiftWindowMSA, WindowAttentionFunction, convert_hip_window_attention, window_attention, window_attention_backward,
                   window_attention_torch)
from .linear import HipFFN, convert_hip_swin_linears, linear_forward, pack_weight

__all__ = [
    "DDIMScheduler", "HipDenoiser", "precision_id", "library_path", "load_library",
    "ScheduledCNNRefine", "CNNDDIMPipiline", "DeepDepthTransformWithUpsampling",
    "DDIMDepthEstimate_Res", "DDIMDepthEstimate_Swin_ADD", "DDIMDepthEstimate_Swin_ADDHAHI", "DDIMDepthEstimate_MPVIT_ADDHAHI",
    "DDIMDepthEstimate_ResVis", "DDIMDepthEstimate_Swin_ADDHAHIVis", "HAHIHeteroNeck", "NLSPN", "Diffusion_DCbase_Model",
    "Diffusion_DCbase_Metric", "MetricAccumulator", "Diffusion_DCbase_Loss",
    "HipBatchNorm2d", "convert_hip_batchnorm", "fuse_basic_block_tails", "HipConv2d", "HipConvTranspose2d", "convert_hip_conv",
    "HipCodecConv2d", "HipCodecConvTranspose2d", "HipCodecTail", "convert_hip_codec", "fuse_conv_bn_stats", "conv_bn_train",
    "HipShiftWindowMSA", "convert_hip_window_attention", "window_attention", "window_attention_torch", "WindowAttentionFunction",
    "window_attention_backward", "HipFFN", "convert_hip_swin_linears", "linear_forward", "pack_weight",
]
__version__ = "0.1.0"
