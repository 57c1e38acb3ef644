"""On-disk compression of trained splats (reference gsplat/compression/)."""
from .png_compression import PngCompression, kmeans_assign_l1, kmeans_l1

__all__ = ["PngCompression", "kmeans_l1", "kmeans_assign_l1"]
