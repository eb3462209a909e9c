"""cvpr23_lfdm_amd - MI355X-native LFDM sampling + DM-training path.

Public surface mirrors the reference's classes:
  FlowDiffusion (DM/modules/video_flow_diffusion_model.py), Unet3D / GaussianDiffusion
  (DM/modules/video_flow_diffusion.py), Generator (LFAE/modules/generator.py).
"""
from . import evaluate  # noqa: F401  (paired video metrics on the device: DESIGN.md 4.6)
from . import retime  # noqa: F401  (frame times for decoding a sample at another frame rate: DESIGN.md 4.9)
from . import video_store  # noqa: F401  (packed uint8 video store, batch preparation on the device: DESIGN.md 4.7)
from .diffusion import GaussianDiffusion  # noqa: F401
from .flow_diffusion import FlowDiffusion, FlowDiffusionFunctional  # noqa: F401
from .generator import Generator  # noqa: F401
from .unet import Unet3D  # noqa: F401
