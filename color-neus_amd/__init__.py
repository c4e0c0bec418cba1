"""MI355X-native volume renderer for Color-NeuS (hand-written HIP kernels behind a C ABI).

Public surface (mirrors the reference's RENDERER plug-in interface, lib/utils/builder.py:309):
    ColorNeuSRenderer / NeuSRenderer   nn.Modules with NeuS.forward's signature and return dict
    RENDERER, build_renderer            registry look-alike; register_into(reference_registry) for drop-in use
    load_library                        the ctypes binding of libcolorneus_hip.so
"""
from .config import RenderConfig, config_from_node  # noqa: F401
from ._lib import load_library, library_path, RenderLibrary  # noqa: F401
from .renderer import ColorNeuSRenderer, NeuSRenderer, RENDERER, build_renderer, register_into, sample_pdf  # noqa: F401
from .loss import compute_loss, compute_loss_fused  # noqa: F401
from . import parallel, rays, synthetic, optim, meshio, metrics, imaging, cameras, meshops, registration  # noqa: F401
from .meshio import write_ply, write_png  # noqa: F401
from .metrics import (nearest_neighbors, chamfer_distance, mesh_metrics, compute_chamfer_distance, point_mesh_distance, surface_metrics,  # noqa: F401
                      compute_surface_metrics)  # noqa: F401
from .imaging import image_metrics, psnr, ssim, mse2psnr, PSNR, SSIM, cmap, panel, validate_image, rasterize_mesh, mesh_view_metrics  # noqa: F401
from .meshops import connected_components, clean_mesh, sample_surface, ViewMasks, dilate_masks, view_votes, cull_mesh, MeshCuller  # noqa: F401
from .registration import icp, Registration, apply_transform  # noqa: F401
from .rays import PixelSampler  # noqa: F401
from .cameras import FocalNet, PoseNet, Cameras, cameras_from_state_dict  # noqa: F401
from .optim import ClipAdam  # noqa: F401

__all__ = ["RenderConfig", "config_from_node", "load_library", "library_path", "RenderLibrary", "ColorNeuSRenderer",
           "NeuSRenderer", "RENDERER", "build_renderer", "register_into", "compute_loss", "compute_loss_fused", "parallel", "rays", "synthetic", "sample_pdf", "optim", "ClipAdam", "meshio", "write_ply",
           "metrics", "nearest_neighbors", "chamfer_distance", "mesh_metrics", "compute_chamfer_distance",
           "point_mesh_distance", "surface_metrics", "compute_surface_metrics", "sample_surface",
           "registration", "icp", "Registration", "apply_transform",
           "imaging", "image_metrics", "psnr", "ssim", "mse2psnr", "PSNR", "SSIM", "cmap", "panel", "validate_image", "rasterize_mesh", "mesh_view_metrics", "write_png",
           "meshops", "connected_components", "clean_mesh", "ViewMasks", "dilate_masks", "view_votes", "cull_mesh", "MeshCuller", "PixelSampler", "cameras", "FocalNet", "PoseNet", "Cameras", "cameras_from_state_dict"]
