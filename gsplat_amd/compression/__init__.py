"""On-disk compression of trained splats (reference gsplat/compression/)."""
from .png_compression import PngCompression, kmeans_assign_l1, kmeans_l1
from .sort import plas_sort

__all__ = ["PngCompression", "kmeans_l1", "kmeans_assign_l1", "plas_sort"]
