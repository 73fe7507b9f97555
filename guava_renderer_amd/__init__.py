"""guava_renderer_amd: the gfx950 renderer and avatar operations.  Submodules import torch and
load the library on first use; the names below are resolved lazily so that importing the package
stays free of both."""

_LAZY = {"UVGaussianExtractor": "gaussian_extract", "StyleDecoder": "refiner", "StyleUNetRunner": "refiner"}

__all__ = sorted(_LAZY)


def __getattr__(name):
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module("." + _LAZY[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
