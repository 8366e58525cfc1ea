"""Drop-in for the reference's ``nvdiffrast`` dependency (``import nvdiffrast.torch as dr``,
/root/reference/lib/models/sky_cubemap.py:7): only ``nvdiffrast.torch.texture`` for cube maps, the one call the
reference's sky model makes (street_gaussians_amd/texture.py)."""
