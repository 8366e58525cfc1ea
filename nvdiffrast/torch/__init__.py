"""``nvdiffrast.torch`` as the reference's sky model uses it: ``texture`` with ``boundary_mode='cube'`` and bilinear
filtering, on the MI355X-native kernels of street_gaussians_amd.texture.  Every other attribute of nvdiffrast.torch
(``rasterize``, ``interpolate``, ``antialias``, ``RasterizeCudaContext``, ...) raises NotImplementedError."""
from street_gaussians_amd.texture import texture  # noqa: F401


def __getattr__(name):
    if name.startswith("__"):
        raise AttributeError(name)
    raise NotImplementedError(f"nvdiffrast.torch.{name} is not implemented: this drop-in provides only texture() with "
                              "boundary_mode='cube' and bilinear filtering")
