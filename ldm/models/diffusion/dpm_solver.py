from adaface_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler  # noqa: F401
