"""splat_renderer_amd — MI355X-native tile-raster hot path of ath92/splat-renderer.

HIP kernels (csrc/) behind the C ABI in include/splat.h, plus host classes that keep the
reference's Renderer/Camera/PointManager/SplatPropertyManager + stage-class surface (host.py).
Importing the package does not need a GPU; creating a Device does (there is no CPU fallback).
"""
from . import scene  # noqa: F401
from ._lib import (MODE_FRONT_TO_BACK, MODE_REFERENCE_LITERAL, STAGE_BIN, STAGE_COMPOSITE, STAGE_NAMES,  # noqa: F401
                   STAGE_PROJECT, STAGE_SORT, CompositeCfg, SplatError)
from .camera import Camera  # noqa: F401
from .host import (Buffer, CommandEncoder, ComputeShaderRenderer, DepthKeyExtractor, Device, GaussianCloud, GPUTileBinner,  # noqa: F401
                   PerTileSorter, PipelinedRenderer, PointManager, PointRenderer, PrefixSumScanner, PropertyPlanes, RadixSorter, Renderer, SequentialRenderer,
                   SplatProjector, SplatPropertyManager, TileRenderer)
from .frameloop import FrameLoop, MouseEvent, OrbitCameraController, SdfSplatSource, read_png, write_png  # noqa: F401
from . import sdf  # noqa: F401
from .ply import load_gaussian_ply, load_point_ply, load_surfel_ply, save_gaussian_ply, save_mesh_ply, save_surfel_ply  # noqa: F401
from .fit import GaussianFit, SurfelFit  # noqa: F401
from .tsdf import TsdfVolume  # noqa: F401  (torch is imported when a volume is first made)
from .autograd import depth_normals, normal_consistency_loss, splat_normals  # noqa: F401  (torch is imported when one is first called)
from .autograd import project_surfels, render_surfels, surfel_normals  # noqa: F401  (2D Gaussian surfels: autograd's docstring)


def knn_mean_sq_distance(points, return_evaluations=False):
    """autograd.knn_mean_sq_distance (torch is imported when it is first called)."""
    from .autograd import knn_mean_sq_distance as f
    return f(points, return_evaluations)


from .sdf import CurvatureSampler, GradientSampler, PositionUpdater, SDFScene  # noqa: F401
