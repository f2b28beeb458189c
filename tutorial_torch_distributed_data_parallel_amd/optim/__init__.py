"""Fused optimizers (native single-pass kernels on GPU; torch semantics), and the layer-wise
adaptive LAMB / LARS (three launches: per-tensor norms, then the update)."""
from .fused import LAMB, LARS, SGD, Adam, AdamW

__all__ = ["SGD", "Adam", "AdamW", "LAMB", "LARS"]
