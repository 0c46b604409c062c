"""rollingdepth_amd — RollingDepth's snippet-denoise hot path on AMD MI355X (gfx950).

Public surface mirrors the reference: RollingDepthPipeline / RollingDepthOutput
(rollingdepth/rollingdepth_pipeline.py), DepthAligner (rollingdepth/depth_aligner.py) and the
modified diffusers attention processor (CrossFrameAttnProcessor); depth_metrics / align_scale_shift
(metrics.py) score a depth video after a least-squares scale and shift, temporal_metrics its change
from frame to frame, boundary_metrics the precision and recall of its occlusion boundaries; optical_flow
(flow.py) estimates the flow and occlusion mask the temporal score needs from the RGB frames; quantiles (kernels.py) takes exact order statistics of a device tensor; guided_upsample (upsample.py)
brings a depth video to the frames' resolution with its edges on the image's; temporal_filter (stabilize.py)
averages a depth video along the optical flow to take out its flicker.  All arithmetic runs in
librdmi.so (HIP); importing the compute modules without the built library raises.
"""
__version__ = "0.1.0"


def __getattr__(name):
    if name in ("RollingDepthPipeline", "RollingDepthOutput"):
        from . import pipeline
        return getattr(pipeline, name)
    if name == "DepthAligner":
        from .aligner import DepthAligner
        return DepthAligner
    if name == "CrossFrameAttnProcessor":
        from .attention_processor import CrossFrameAttnProcessor
        return CrossFrameAttnProcessor
    if name in ("depth_metrics", "align_scale_shift", "DepthMetrics", "temporal_metrics", "TemporalMetrics",
                "boundary_metrics", "BoundaryMetrics"):
        from . import metrics
        return getattr(metrics, name)
    if name in ("optical_flow", "OpticalFlow"):
        from . import flow
        return getattr(flow, name)
    if name == "guided_upsample":
        from .upsample import guided_upsample
        return guided_upsample
    if name == "temporal_filter":
        from .stabilize import temporal_filter
        return temporal_filter
    if name == "quantiles":
        from .kernels import quantiles
        return quantiles
    raise AttributeError(name)
