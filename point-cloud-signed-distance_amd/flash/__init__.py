"""flash — MI355X-native residual pass of Flash.jl (host package).

Module layout mirrors `module Flash` (src/Flash.jl): core types and
`skin(state)` here, submodules `Models`, `GradientDescent`, `Tracking`.
The compute path is libflashsdf.so (HIP, gfx950) through ctypes; there is no
CPU fallback.
"""
from .core import (BodyGeometry, ConvexGeometry, DeformableInterpolatingSkin, InterpolatingGeometry,
                   Manipulator, ManipulatorState, RigidInterpolatingSkin, SceneSkin, hull_poses,
                   num_deformations, num_states, skin, surfaces)
from . import models as Models  # noqa: N812
from ._lib import FlashNativeError
from .robust import Huber, Tukey

__all__ = ["BodyGeometry", "ConvexGeometry", "DeformableInterpolatingSkin", "InterpolatingGeometry",
           "Manipulator", "ManipulatorState", "RigidInterpolatingSkin", "SceneSkin", "hull_poses",
           "num_deformations", "num_states", "skin", "surfaces", "Models", "FlashNativeError",
           "LevenbergMarquardt", "Huber", "Tukey", "depth_noise_weights", "DepthFrame", "FreeSpace",
           "VoxelGrid", "multi_start", "candidates_around"]


def __getattr__(name):
    # GradientDescent / Tracking import lazily (they pull in the solver)
    if name == "GradientDescent":
        from . import gradientdescent
        return gradientdescent
    if name == "Tracking":
        from . import tracking
        return tracking
    if name == "LevenbergMarquardt":  # the opt-in second-order tracking solver
        from .tracking import LevenbergMarquardt
        return LevenbergMarquardt
    if name in ("multi_start", "candidates_around"):  # a start found by scoring many candidates at once
        from . import tracking
        return getattr(tracking, name)
    if name == "depth_noise_weights":  # per-point confidence weights from a depth sensor's axial noise
        from .depthsensors import depth_noise_weights
        return depth_noise_weights
    if name == "DepthFrame":  # a depth image, its sensor and pose, taken wherever a sensed cloud is
        from .depthsensors import DepthFrame
        return DepthFrame
    if name == "FreeSpace":  # a depth frame's free-space samples (DepthFrame(..., free_space=FreeSpace(...)))
        from .depthsensors import FreeSpace
        return FreeSpace
    if name == "VoxelGrid":  # a world-anchored voxel grid that thins a cloud or depth frame (`voxel=`)
        from .depthdata import VoxelGrid
        return VoxelGrid
    if name == "DepthSensors":
        from . import depthsensors
        return depthsensors
    if name == "DepthData":
        from . import depthdata
        return depthdata
    raise AttributeError(name)
