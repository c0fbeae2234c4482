"""Public names of the package (see ml_gmpi_amd/__init__.py for why this is not an __init__)."""
from ._lib import GmpiError, build_extension, library_path, load_library
from .hip_mpi import MPI, HipMPI, ChunkedRender, flush_status
from .renderer import MPIRenderer, PRESETS, make_renderer, rays_from_c2w
from .driver import ViewBatchDriver, shard_views, render_views_sharded, frames_to_uint8, dump_frames
from .install import install, uninstall
from .light import LightRenderer, compute_depth, compute_depth_ramp
from .shared_color import expand_shared_color, split_shared_color
from .shaded import apply_shading
from .depth_alpha import depth_alpha_bounds, depth_alpha_planes, expand_depth_alpha
from .quantized import quantize_volume, dequantize_volume, layers_as_volume, volume_as_layers
from .layers import is_float_layers
from .occupancy import Occupancy, build_occupancy, occupancy_reference

__all__ = [
    "GmpiError", "build_extension", "library_path", "load_library",
    "MPI", "HipMPI", "ChunkedRender", "flush_status", "MPIRenderer", "PRESETS", "make_renderer", "rays_from_c2w",
    "ViewBatchDriver", "shard_views", "render_views_sharded", "frames_to_uint8", "dump_frames",
    "install", "uninstall", "compute_depth", "compute_depth_ramp", "LightRenderer", "expand_shared_color", "split_shared_color",
    "apply_shading",
    "depth_alpha_bounds", "depth_alpha_planes", "expand_depth_alpha",
    "quantize_volume", "dequantize_volume", "layers_as_volume", "volume_as_layers",
    "is_float_layers",
    "Occupancy", "build_occupancy", "occupancy_reference",
]
