from adaface_amd.ldm.modules.diffusionmodules.controlnet import ControlNet  # noqa: F401
