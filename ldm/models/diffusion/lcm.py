from adaface_amd.ldm.models.diffusion.lcm import LCMSampler  # noqa: F401
