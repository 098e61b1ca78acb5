#!/usr/bin/env python
"""MI355X counterpart of the reference's scripts/stable_txt2img.py (the caller of the hot path).

Keeps the reference's flag names for everything that reaches the denoising path
(stable_txt2img.py:38-310): --config --ckpt --n_samples --n_repeat --ddim_steps --ddim_eta --scale --H --W --C --f
--seed --outdir --skip_save --fixed_code --gpu --bs --plms --dpm_solver --dpm_sde --lcm --tcd_gamma --noise --deep_cache --init_img_paths --init_img_weight.  Text conditioning is the one difference: the CLIP tower /
EmbeddingManager are out of scope offline, so prompts are given as pre-computed embeddings
(--prompt_emb file.pt/.npy with a [B*16,77,768] or [77,768] tensor) or --synthetic.
Not in the reference: --img2img / --strength / --inpaint_mask (img2img by strength and inpainting, adaface_amd/img2img.py);
--hires_scale / --hires_size / --hires_upscaler / --hires_strength / --hires_steps (hires fix, adaface_amd/hires.py).

    python scripts/stable_txt2img.py --synthetic --n_samples 8 --ddim_steps 50 --skip_save
    python scripts/stable_txt2img.py --synthetic --n_samples 64 --gpus 8      # starts the 8 ranks itself
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 scripts/stable_txt2img.py --synthetic --n_samples 64 --gpus 8
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, default=None, help="reference yaml (v1-inference-ada.yaml); default: built-in SD-1.5")
    ap.add_argument("--ckpt", type=str, default=None, help="SD checkpoint (.ckpt / .safetensors); default: seeded synthetic weights")
    ap.add_argument("--prompt_emb", type=str, default=None, help="pre-computed conditional embedding (.pt / .npy)")
    ap.add_argument("--neg_prompt_emb", type=str, default=None, help="pre-computed unconditional embedding")
    ap.add_argument("--synthetic", action="store_true", help="synthetic N(0,1) context of the reference's shape")
    ap.add_argument("--outdir", type=str, default="outputs/txt2img-samples")
    ap.add_argument("--skip_save", action="store_true", help="do not save individual samples (speed measurements)")
    ap.add_argument("--ddim_steps", type=int, default=50)
    ap.add_argument("--ddim_eta", type=float, default=0.0)
    ap.add_argument("--fixed_code", action="store_true", help="same starting code across repeats")
    ap.add_argument("--n_repeat", type=int, default=1)
    ap.add_argument("--n_samples", "--bs", dest="n_samples", type=int, default=8, help="global batch (sharded over ranks)")
    ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--W", type=int, default=512)
    ap.add_argument("--C", type=int, default=4)
    ap.add_argument("--f", type=int, default=8)
    ap.add_argument("--scale", type=float, nargs="+", default=[10.0, 4.0], help="guidance scale, or max min for annealing")
    ap.add_argument("--init_img_paths", type=str, nargs="+", default=None,
                    help="initial image(s): encoded by the VAE encoder, averaged, blended with noise into the start code")
    ap.add_argument("--init_img_weight", type=float, default=0.1, help="w: start = w*enc(img) + (1-w)*noise")
    smp = ap.add_mutually_exclusive_group()
    smp.add_argument("--plms", action="store_true", help="PLMS sampler instead of DDIM (scalar --scale)")
    smp.add_argument("--dpm_solver", action="store_true",
                     help="DPM-Solver++(2M) sampler instead of DDIM: made for 15-25 --ddim_steps (eta must be 0)")
    smp.add_argument("--lcm", action="store_true",
                     help="LCM sampler instead of DDIM, for a consistency-distilled model or an LCM-LoRA (--lora lcm-lora.safetensors "
                          "--scale 1.5): made for 2-8 --ddim_steps (eta must be 0)")
    ap.add_argument("--lcm_original_steps", type=int, default=50, metavar="N",
                    help="--lcm: the solver steps of the distillation; the grid is thinned from the N timesteps (i + 1) 1000 / N - 1")
    ap.add_argument("--tcd_gamma", type=float, default=None, metavar="G",
                    help="TCD sampling on the LCM grid, G in [0, 1]: 0 = deterministic (DDIM), 1 = the LCM re-noising; implies --lcm")
    ap.add_argument("--lcm_guidance_embedding", action="store_true",
                    help="--lcm: feed --scale (one number) through the checkpoint's guidance-scale embedding (a config with "
                         "time_cond_proj_dim) and run one U-Net leg per step, as a fully distilled LCM checkpoint expects")
    ap.add_argument("--dpm_skip", choices=["time_uniform", "logSNR"], default="time_uniform",
                    help="--dpm_solver: the timestep grid; time_uniform = DDIM's, logSNR = uniform in log(alpha / sigma)")
    ap.add_argument("--dpm_sde", action="store_true",
                    help="--dpm_solver: the stochastic variant, DPM-Solver++(2M) SDE (one noise draw per step, in the step kernel)")
    ap.add_argument("--noise", choices=["torch", "philox"], default="torch",
                    help="where the start code and the samplers' noise come from.  torch: the start code from the seeded host "
                         "generator, step noise (--ddim_eta > 0, --dpm_sde) from the device's default generator, which --seed "
                         "does not reach.  philox: all of it keyed by (--seed, global sample index, step): --seed names an image "
                         "whatever the batch split or --gpus")
    ap.add_argument("--deep_cache", type=int, default=None, metavar="N",
                    help="DeepCache: the full U-Net on every N-th step only; between them its outermost blocks run on the deep "
                         "feature kept at the last full step (DDIM and --dpm_solver; 1 = off)")
    ap.add_argument("--deep_cache_depth", type=int, default=2, metavar="K",
                    help="--deep_cache: input / output blocks that still run on the steps between (1 .. 11 for SD-1.5)")
    ap.add_argument("--tome", type=float, default=0.0, metavar="RATIO",
                    help="token merging in front of the U-Net's self-attention: the share of a map's tokens merged away, "
                         "0 .. 0.75 (0 = off); composes with every sampler, --deep_cache and --gpus; --dtype bf16 / f32")
    ap.add_argument("--tome_max_downsample", type=int, default=1, choices=[1, 2],
                    help="--tome: 1 = the 64x64-level transformers only, 2 = the 32x32 level too")
    ap.add_argument("--freeu", type=float, nargs=4, default=None, metavar=("B1", "B2", "S1", "S2"),
                    help="FreeU: backbone factors B1, B2 in [1, 2] and skip factors S1, S2 in [0, 1] (SD-1.5: 1.2 1.4 0.9 0.2, "
                         "version 2: 1.3 1.4 0.9 0.2); composes with every sampler, --dtype, --deep_cache, --tome and --gpus")
    ap.add_argument("--freeu_version", type=int, default=1, choices=[1, 2],
                    help="--freeu: 1 = a constant backbone factor, 2 = the factor follows the backbone's channel mean")
    ap.add_argument("--pag_scale", type=float, default=0.0, metavar="S",
                    help="perturbed-attention guidance: e += S (e_cond - e_perturbed), a third U-Net leg per step whose "
                         "self-attention maps at --pag_layers are the identity (0 = off; diffusers' SD-1.5 default is 3); composes "
                         "with every sampler, --dtype, --deep_cache, --freeu, --gpus, and --tome where no merging level is a PAG layer")
    ap.add_argument("--pag_layers", type=str, nargs="+", default=None, metavar="LAYER",
                    help="--pag_scale: mid, down.blocks.0..2, up.blocks.1..3 or site numbers 0..15 (default: mid)")
    ap.add_argument("--pag_adaptive_scale", type=float, default=0.0, metavar="A",
                    help="--pag_scale: the scale of the step at timestep t is max(S - A (1000 - t), 0)")
    ap.add_argument("--guidance_rescale", type=float, default=0.0, metavar="PHI",
                    help="guidance rescale, 0 .. 1 (0 = off): the combined prediction is scaled towards the conditional one's "
                         "standard deviation, the remedy for over-exposure at high guidance; every sampler")
    ap.add_argument("--sag_scale", type=float, default=0.0, metavar="S",
                    help="self-attention guidance: e += S (e_guide - e_degraded), one more single-leg U-Net call per step on the "
                         "input blurred where the middle block's self-attention looks (0 = off; diffusers' default is 0.75); works "
                         "with --scale 1 too.  DDIM, --plms and --dpm_solver; composes with --dtype bf16 / f32 / fp16, --lora, --freeu, "
                         "--img2img, --inpaint_mask, --noise philox, --gpus, and --tome where the middle block does not merge; not with "
                         "--pag_scale, --guidance_rescale, --tgate, --deep_cache, --controlnet, regional prompts, --lcm or --dtype fp8")
    ap.add_argument("--sag_blur_sigma", type=float, default=1.0, metavar="F",
                    help="--sag_scale: the sigma of the 9-tap Gaussian blur, F > 0 (default 1.0)")
    ap.add_argument("--tgate", type=int, default=None, metavar="G",
                    help="T-GATE: step G - 1 also keeps the cross-attention outputs (averaged over the guidance legs); from step G "
                         "on the U-Net runs on one leg with them, without cross-attention or guidance; 1 <= G <= steps - 1 "
                         "(0 = off).  DDIM and --dpm_solver; composes with --deep_cache, --tome, --freeu, --lora and --gpus; not "
                         "with --plms, --pag_scale, --guidance_rescale or --dtype fp8")
    ap.add_argument("--lora", type=str, action="append", default=None, metavar="PATH[:SCALE]",
                    help="LoRA adapter file (.safetensors / .pt, kohya or native key names) merged into the U-Net's and the text "
                         "tower's weights as they are repacked; repeatable, at most 8; SCALE defaults to 1; composes with every "
                         "sampler, --dtype, --deep_cache, --tome, --freeu, --pag_scale and --gpus")
    ap.add_argument("--controlnet", type=str, default=None, metavar="PATH[:SCALE]",
                    help="ControlNet checkpoint (control_sd15_*.pth / control_v11p_sd15_*.pth|.safetensors, keys with or without "
                         "control_model.), or `synthetic` for seeded synthetic weights; SCALE (default 1) multiplies every residual.  "
                         "Composes with every sampler, --lora (not applied to the control branch), --tome (U-Net only), --freeu, "
                         "--deep_cache, --gpus and every --dtype (fp8: the control branch runs in bf16); not with --pag_scale or --tgate")
    ap.add_argument("--control_image", type=str, nargs="+", default=None, metavar="PATH",
                    help="--controlnet: the hint image(s), resized to H x W: one for all samples, or one per global sample index")
    ap.add_argument("--control_start", type=float, default=0.0, metavar="F",
                    help="--controlnet: control is on from this fraction of the schedule (0 = the first step) ...")
    ap.add_argument("--control_end", type=float, default=1.0, metavar="F",
                    help="... to this one (1 = the last step): timesteps 999 (1 - END) .. 999 (1 - START)")
    ap.add_argument("--control_cond_only", action="store_true",
                    help="--controlnet: control on the conditional guidance leg only (the unconditional leg is left as it is)")
    ap.add_argument("--region_emb", type=str, nargs="+", default=None, metavar="PATH",
                    help="regional prompts: one pre-computed embedding per region, as --prompt_emb (which stays the base prompt, "
                         "heard everywhere at --region_base_weight); with --region_box or --region_mask, one per embedding.  At most "
                         "7 regions.  Composes with every sampler, --dtype, --deep_cache, --tome, --freeu, --lora, --img2img, "
                         "--inpaint_mask, --noise philox and --gpus; not with --pag_scale, --tgate or --controlnet")
    ap.add_argument("--region_box", type=str, nargs="+", default=None, metavar="X0,Y0,X1,Y1[:W]",
                    help="--region_emb: the regions as boxes in image fractions, optionally with a weight (default 1)")
    ap.add_argument("--region_mask", type=str, nargs="+", default=None, metavar="IMG",
                    help="--region_emb: the regions as mask images (white = the region), area-averaged to the latent grid")
    ap.add_argument("--region_base_weight", type=float, default=0.2, metavar="F",
                    help="regional prompts: the weight of the base prompt in every latent cell (the regions' weights are their masks)")
    ap.add_argument("--regions", type=str, default=None, metavar="synthetic:N",
                    help="regional prompts without files: N seeded synthetic region contexts on N vertical strips")
    ap.add_argument("--img2img", type=str, nargs="+", default=None, metavar="PATH",
                    help="img2img by strength: the image(s) to start from, resized to H x W: one for all samples, or one per "
                         "global sample index.  The run executes the last --strength share of the schedule from the noised "
                         "encoding.  Composes with every sampler, --dtype, --noise, --deep_cache, --tome, --freeu, --lora, "
                         "--gpus and --controlnet; not with --init_img_paths")
    ap.add_argument("--strength", type=float, default=None, metavar="F",
                    help="--img2img: in (0, 1], the share of the steps that run (1 = all of them, from pure noise plus the "
                         "image's trace; default 0.75)")
    ap.add_argument("--inpaint_mask", type=str, nargs="+", default=None, metavar="PATH",
                    help="--img2img: inpainting mask(s), white = repaint, resized to H x W: one for all samples, or one per "
                         "global sample index.  A latent cell with any white pixel is repainted; the rest is the image's own "
                         "encoding.  A checkpoint or config with a 9-channel U-Net (sd-v1-5-inpainting) needs it")
    ap.add_argument("--hires_scale", type=float, default=None, metavar="F",
                    help="hires fix: --H x --W is the first pass's size; its result is upscaled by F in (1, 4] (each latent side "
                         "rounded to a multiple of 8) and a second img2img pass runs at that size.  Composes with every sampler, "
                         "--dtype bf16 / f32 / fp16, --deep_cache, --tome, --freeu, --lora, --pag_scale, --guidance_rescale, "
                         "--sag_scale, --tgate, --lcm, --noise philox and --gpus; not with --img2img, --inpaint_mask, --controlnet, "
                         "regional prompts, --init_img_paths or --dtype fp8")
    ap.add_argument("--hires_size", type=int, nargs=2, default=None, metavar=("H", "W"),
                    help="hires fix by target size in pixels instead of --hires_scale: multiples of 64, no smaller than --H x --W")
    ap.add_argument("--hires_upscaler", choices=["latent", "latent-bicubic", "latent-nearest", "pixel-bicubic", "pixel-lanczos"],
                    default="latent",
                    help="hires fix: latent* resample the latent (bilinear / bicubic / nearest); pixel-* decode, resample the "
                         "image (bicubic / Lanczos-3) and encode it again")
    ap.add_argument("--hires_strength", type=float, default=0.7, metavar="F",
                    help="hires fix: the share of the second pass's schedule that runs, in (0, 1] (default 0.7)")
    ap.add_argument("--hires_steps", type=int, default=0, metavar="N",
                    help="hires fix: the second pass's schedule length (0 = --ddim_steps)")
    ap.add_argument("--lora_strict", action="store_true", help="--lora: refuse a file with keys that map onto no layer")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--gpu", type=int, default=None)
    ap.add_argument("--gpus", type=int, default=1,
                    help="data-parallel ranks (one process per GPU); without a launcher the ranks are started here")
    ap.add_argument("--dtype", choices=["bf16", "f32", "fp16", "fp8"], default="bf16",
                    help="fp16: fp16 storage on the f16 MFMA, the precision of the reference's autocast path; "
                         "fp8: bf16 with the UNet's ResBlock convolutions and self-attention q/k/v on e4m3 operands (PARITY UNPINNED)")
    ap.add_argument("--fp8-scope", dest="fp8_scope", choices=["base", "base+ff"], default="base",
                    help="--dtype fp8: base = ResBlock convolutions + self-attention q/k/v; base+ff = also the transformer "
                         "blocks' FeedForward (GEGLU + ff.net.2).  A scale file belongs to the scope it was calibrated under")
    ap.add_argument("--fp8_calib_steps", type=int, default=10,
                    help="--dtype fp8: DDIM steps of the calibration sample that sets the per-layer activation scales "
                         "(two passes, with this run's conditioning); 0 = keep the fixed 2^3, which clips beyond +-56")
    ap.add_argument("--fp8_scales", type=str, default=None,
                    help="--dtype fp8: JSON file of calibrated scales: loaded if present, else written after the calibration")
    opt = ap.parse_args(argv)
    if opt.dpm_sde and not opt.dpm_solver:
        ap.error("--dpm_sde is a variant of --dpm_solver: give both")
    if opt.tcd_gamma is not None:
        if opt.plms or opt.dpm_solver:
            ap.error("--tcd_gamma: implies --lcm, which is not allowed with --plms or --dpm_solver")
        if not 0.0 <= opt.tcd_gamma <= 1.0:
            ap.error("--tcd_gamma G: 0 <= G <= 1")
        opt.lcm = True
    if (opt.lcm_guidance_embedding or opt.lcm_original_steps != 50) and not opt.lcm:
        ap.error("--lcm_guidance_embedding / --lcm_original_steps: give --lcm too")
    if opt.lcm:
        if not 1 <= opt.lcm_original_steps <= 1000:
            ap.error("--lcm_original_steps N: 1 <= N <= 1000")
        if not 1 <= opt.ddim_steps <= opt.lcm_original_steps:
            ap.error(f"--lcm: 1 <= --ddim_steps <= --lcm_original_steps ({opt.lcm_original_steps})")
        if opt.ddim_eta != 0.0:
            ap.error("--lcm: --ddim_eta has no meaning for the consistency update (its noise is the sampler's own)")
        if opt.deep_cache not in (None, 1) or opt.tgate:
            ap.error("--lcm: --deep_cache and --tgate target long schedules and are not built for it")
        if opt.lcm_guidance_embedding and len(opt.scale) != 1:
            ap.error("--lcm_guidance_embedding: --scale must be one number (the embedding is constant over a run)")
        if opt.lcm_guidance_embedding and (opt.pag_scale > 0.0 or opt.guidance_rescale > 0.0):
            ap.error("--lcm_guidance_embedding: the run has one leg per step, so --pag_scale / --guidance_rescale have nothing to act on")
    if opt.deep_cache is not None and opt.deep_cache < 1:
        ap.error("--deep_cache N: N >= 1")
    if opt.deep_cache not in (None, 1) and opt.plms:
        ap.error("--deep_cache: PLMS calls the model twice in its first step and keeps an eps history (use DDIM or --dpm_solver)")
    if not 0.0 <= opt.tome <= 0.75:
        ap.error("--tome RATIO: 0 <= RATIO <= 0.75")
    if opt.tome > 0.0 and opt.dtype in ("fp16", "fp8"):
        ap.error("--tome: token merging runs with --dtype bf16 or f32")
    if opt.freeu is not None:
        b1, b2, s1, s2 = opt.freeu
        if not (1.0 <= b1 <= 2.0 and 1.0 <= b2 <= 2.0):
            ap.error("--freeu B1 B2 S1 S2: 1 <= B1, B2 <= 2")
        if not (0.0 <= s1 <= 1.0 and 0.0 <= s2 <= 1.0):
            ap.error("--freeu B1 B2 S1 S2: 0 <= S1, S2 <= 1")
    if opt.pag_scale < 0.0 or opt.pag_adaptive_scale < 0.0:
        ap.error("--pag_scale S, --pag_adaptive_scale A: S, A >= 0")
    if not 0.0 <= opt.guidance_rescale <= 1.0:
        ap.error("--guidance_rescale PHI: 0 <= PHI <= 1")
    if opt.pag_scale == 0.0 and (opt.pag_layers is not None or opt.pag_adaptive_scale > 0.0):
        ap.error("--pag_layers / --pag_adaptive_scale: give --pag_scale S > 0 too")
    if opt.pag_scale > 0.0:
        from adaface_amd.configs import sd15_config
        from adaface_amd.engine import pag_layout, pag_sites_of
        layers = [int(v) if v.lstrip("-").isdigit() else v for v in (opt.pag_layers or ["mid"])]
        if not opt.config:        # (a --config names its own U-Net: its layers are checked when the model is built)
            unet = sd15_config()["model"]["params"]["unet_config"]["params"]
            try:
                sites = pag_sites_of(unet, layers)
            except ValueError as e:
                ap.error(f"--pag_layers: {e}")
            lay = pag_layout(unet)
            merging = [s for s in sites if opt.tome > 0.0 and lay["ds"][s] <= opt.tome_max_downsample]
            if merging:
                ap.error(f"--pag_layers: --tome merges tokens at sites {merging}; a merged self-attention cannot be perturbed")
        opt.pag_layers = layers
    if not (opt.sag_scale >= 0.0 and opt.sag_scale != float("inf")):
        ap.error("--sag_scale S: a finite S >= 0")
    if not (opt.sag_blur_sigma > 0.0 and opt.sag_blur_sigma != float("inf")):
        ap.error("--sag_blur_sigma F: a finite F > 0")
    if opt.sag_scale == 0.0 and opt.sag_blur_sigma != 1.0:
        ap.error("--sag_blur_sigma: give --sag_scale S > 0 too")
    if opt.sag_scale > 0.0:
        if opt.pag_scale > 0.0:
            ap.error("--sag_scale: not with --pag_scale (both perturb or read the middle block's self-attention)")
        if opt.guidance_rescale > 0.0:
            ap.error("--sag_scale: not with --guidance_rescale (its reference is the CFG combine alone)")
        if opt.tgate:
            ap.error("--sag_scale: not built for T-GATE (--tgate): the degraded leg has no cached cross-attention")
        if opt.deep_cache not in (None, 1):
            ap.error("--sag_scale: not with --deep_cache (a reuse step does not run the middle block, so there is no map)")
        if opt.controlnet:
            ap.error("--sag_scale: not built for a ControlNet (--controlnet)")
        if opt.regions is not None or opt.region_emb:
            ap.error("--sag_scale: not built for regional prompts (--regions / --region_emb)")
        if opt.lcm:
            ap.error("--sag_scale: not built for --lcm (a distilled model runs without guidance legs)")
        if opt.dtype == "fp8":
            ap.error("--sag_scale: not built for --dtype fp8")
        if opt.tome > 0.0 and not opt.config:
            from adaface_amd.configs import sd15_config
            unet = sd15_config()["model"]["params"]["unet_config"]["params"]
            if 2 ** (len(unet["channel_mult"]) - 1) <= opt.tome_max_downsample:
                ap.error("--sag_scale: --tome merges tokens at the middle block, whose attention then has no map over the full grid")
        if (opt.H // opt.f) % 8 or (opt.W // opt.f) % 8 or opt.H % opt.f or opt.W % opt.f:
            ap.error("--sag_scale: the latent sides (--H / --f, --W / --f) must be multiples of 8")
    if opt.tgate is not None and opt.tgate < 0:
        ap.error("--tgate G: G >= 1 (0 = off)")
    if opt.tgate:
        if opt.plms:
            ap.error("--tgate: PLMS keeps an eps history across the gate (use DDIM or --dpm_solver)")
        if opt.pag_scale > 0.0 or opt.guidance_rescale > 0.0:
            ap.error("--tgate: after the gate no guidance combine is made, so --pag_scale / --guidance_rescale have nothing to act on")
        if opt.dtype == "fp8":
            ap.error("--tgate: not built for --dtype fp8")
    control_extras = opt.control_image is not None or opt.control_cond_only or opt.control_start != 0.0 or opt.control_end != 1.0
    if control_extras and not opt.controlnet:
        ap.error("--control_image / --control_start / --control_end / --control_cond_only: give --controlnet PATH[:SCALE] too")
    if opt.controlnet:
        from adaface_amd.engine import control_window_from_fractions
        from adaface_amd.lora import parse_lora_arg
        if opt.pag_scale > 0.0:
            ap.error("--controlnet: not built for the PAG form (--pag_scale)")
        if opt.tgate:
            ap.error("--controlnet: not built for T-GATE (--tgate)")
        path, scale = parse_lora_arg(opt.controlnet)
        if scale != scale or scale in (float("inf"), float("-inf")):
            ap.error(f"--controlnet {path}: the scale must be a finite number")
        if path != "synthetic" and not opt.control_image:
            ap.error("--controlnet: give --control_image PATH [PATH ...] (only `synthetic` makes its own hint)")
        if opt.control_image and len(opt.control_image) not in (1, opt.n_samples):
            ap.error(f"--control_image: one image, or one per sample ({opt.n_samples}), got {len(opt.control_image)}")
        try:
            opt.control_t_range = control_window_from_fractions(opt.control_start, opt.control_end)
        except ValueError as e:
            ap.error(f"--control_start / --control_end: {e}")
        opt.controlnet = (path, scale)
    opt.region_n = 0
    if opt.regions is not None:
        kind, _, n = opt.regions.partition(":")
        if kind != "synthetic" or not n.isdigit() or not 1 <= int(n) <= 7:
            ap.error("--regions synthetic:N with 1 <= N <= 7")
        if opt.region_emb or opt.region_box or opt.region_mask:
            ap.error("--regions synthetic:N makes its own contexts and strips: not with --region_emb / --region_box / --region_mask")
        opt.region_n = int(n)
    if (opt.region_box or opt.region_mask) and not opt.region_emb:
        ap.error("--region_box / --region_mask: give --region_emb PATH [PATH ...] too")
    if opt.region_emb:
        if bool(opt.region_box) == bool(opt.region_mask):
            ap.error("--region_emb: give either --region_box or --region_mask, one per embedding")
        shapes = opt.region_box or opt.region_mask
        if len(shapes) != len(opt.region_emb) or len(shapes) > 7:
            ap.error(f"--region_emb: {len(opt.region_emb)} embeddings but {len(shapes)} boxes / masks (one each, at most 7)")
        if opt.region_box:
            from adaface_amd.regions import parse_box
            try:
                opt.region_box = [parse_box(b) for b in opt.region_box]
            except ValueError as e:
                ap.error(f"--region_box: {e}")
        opt.region_n = len(shapes)
    if opt.region_n:
        which = "--regions" if opt.regions is not None else "--region_emb"
        if opt.pag_scale > 0.0:
            ap.error(f"{which}: not built for the PAG form (--pag_scale)")
        if opt.tgate:
            ap.error(f"{which}: not built for T-GATE (--tgate)")
        if opt.controlnet:
            ap.error(f"{which}: not built for a ControlNet (--controlnet): the control branch has cross-attention of its own")
        if not (opt.region_base_weight >= 0.0 and opt.region_base_weight != float("inf")):
            ap.error("--region_base_weight F: a finite F >= 0")
        if (opt.H // opt.f) % 8 or (opt.W // opt.f) % 8 or opt.H % opt.f or opt.W % opt.f:
            ap.error(f"{which}: the latent sides (--H / --f, --W / --f) must be multiples of 8")
    if opt.strength is not None and not opt.img2img:
        ap.error("--strength: give --img2img PATH [PATH ...] too")
    if opt.inpaint_mask and not opt.img2img:
        ap.error("--inpaint_mask: give --img2img PATH [PATH ...] too (the image whose unmasked region is kept)")
    if opt.img2img:
        if opt.init_img_paths:
            ap.error("--img2img: not with --init_img_paths (that blends the encoding into the start code of a full run)")
        opt.strength = 0.75 if opt.strength is None else opt.strength
        if not 0.0 < opt.strength <= 1.0:
            ap.error("--strength F: 0 < F <= 1")
        for flag, paths in (("--img2img", opt.img2img), ("--inpaint_mask", opt.inpaint_mask)):
            if paths and len(paths) not in (1, opt.n_samples):
                ap.error(f"{flag}: one image, or one per sample ({opt.n_samples}), got {len(paths)}")
        if opt.H % opt.f or opt.W % opt.f:
            ap.error(f"--img2img: --H and --W must be multiples of --f ({opt.f})")
    opt.hires = None
    hires_extras = opt.hires_upscaler != "latent" or opt.hires_strength != 0.7 or opt.hires_steps != 0
    if opt.hires_scale is None and opt.hires_size is None:
        if hires_extras:
            ap.error("--hires_upscaler / --hires_strength / --hires_steps: give --hires_scale F or --hires_size H W too")
    else:
        from adaface_amd import hires as HR
        if opt.hires_scale is not None and opt.hires_size is not None:
            ap.error("--hires_scale / --hires_size: give one of them")
        if opt.H % opt.f or opt.W % opt.f:
            ap.error(f"hires fix: --H and --W must be multiples of --f ({opt.f})")
        if opt.hires_size is not None and any(v < 64 or v % 64 for v in opt.hires_size):
            ap.error("--hires_size H W: positive multiples of 64")
        if not 0.0 < opt.hires_strength <= 1.0:
            ap.error("--hires_strength F: 0 < F <= 1")
        if opt.hires_steps < 0:
            ap.error("--hires_steps N: N >= 0 (0 = --ddim_steps)")
        if opt.lcm and opt.hires_steps > opt.lcm_original_steps:
            ap.error(f"--hires_steps: with --lcm at most --lcm_original_steps ({opt.lcm_original_steps})")
        if opt.img2img or opt.inpaint_mask:
            ap.error("hires fix: not with --img2img / --inpaint_mask (its second pass is the img2img of the first pass's result)")
        if opt.controlnet:
            ap.error("hires fix: not built for a ControlNet (--controlnet): the hint is bound to one size")
        if opt.region_n:
            ap.error("hires fix: not built for regional prompts (--regions / --region_emb): the weight map is bound to one size")
        if opt.init_img_paths:
            ap.error("hires fix: not with --init_img_paths (the blended start code belongs to one size)")
        if opt.dtype == "fp8":
            ap.error("hires fix: not built for --dtype fp8 (the static activation scales are calibrated at one size)")
        try:
            size = None if opt.hires_size is None else (opt.hires_size[0] // opt.f, opt.hires_size[1] // opt.f)
            opt.hires = HR.target_size(opt.H // opt.f, opt.W // opt.f, scale=opt.hires_scale, size=size)
        except ValueError as e:
            ap.error(f"--hires_scale / --hires_size: {e}")
    if opt.noise == "philox" and opt.plms:
        ap.error("--noise philox: PLMS draws no noise and takes no noise source (use DDIM or --dpm_solver)")
    if opt.lora_strict and not opt.lora:
        ap.error("--lora_strict: give --lora PATH[:SCALE] too")
    if opt.lora:
        from adaface_amd.lora import LORA_MAX_ADAPTERS, parse_lora_arg
        if len(opt.lora) > LORA_MAX_ADAPTERS:
            ap.error(f"--lora: at most {LORA_MAX_ADAPTERS} adapters")
        opt.lora = [parse_lora_arg(spec) for spec in opt.lora]
        for path, scale in opt.lora:
            if scale != scale or scale in (float("inf"), float("-inf")):
                ap.error(f"--lora {path}: the scale must be a finite number")
    return opt


def hybrid_problem(opt, hybrid):
    """What keeps a hybrid model (9-channel inpainting U-Net) from running with these options, as a message; None: nothing."""
    if not hybrid:
        return None
    if getattr(opt, "hires", None):
        return "hires fix: not built for a 9-channel (inpainting) U-Net (its concatenated condition is bound to one size)"
    if not (opt.img2img and opt.inpaint_mask):
        return "a 9-channel (inpainting) U-Net needs --img2img PATH and --inpaint_mask PATH: it reads the mask and the masked image"
    if opt.controlnet:
        return "--controlnet: not built for a 9-channel (inpainting) U-Net"
    return None


def load_img(path, h, w):
    """stable_txt2img.py:318-327: RGB, resized to multiples of 32, [-1, 1], NCHW."""
    from PIL import Image
    image = Image.open(path).convert("RGB")
    w, h = (x - x % 32 for x in (w, h))
    image = np.array(image.resize((w, h), resample=Image.LANCZOS)).astype(np.float32) / 255.0
    return 2.0 * torch.from_numpy(image[None].transpose(0, 3, 1, 2)) - 1.0


def load_hint(path, h, w):
    """A ControlNet hint image: RGB, resized to h x w, [0, 1], NCHW."""
    from PIL import Image
    image = np.array(Image.open(path).convert("RGB").resize((w, h), resample=Image.LANCZOS)).astype(np.float32) / 255.0
    return torch.from_numpy(image[None].transpose(0, 3, 1, 2)).clamp(0.0, 1.0)


def load_emb(path, n, device):
    t = torch.tensor(np.load(path)) if path.endswith(".npy") else torch.load(path, map_location="cpu", weights_only=True)
    t = t.float()
    if t.dim() == 2:
        t = t[None].expand(n, -1, -1)
    if t.shape[0] == n:  # [B,77,768] -> layerwise [B*16,77,768] (embedding_manager.py:1342-1353)
        t = t[:, None].expand(n, 16, *t.shape[1:]).reshape(n * 16, *t.shape[1:])
    return t.contiguous().to(device)


def main():
    opt = parse_args()
    import torch.distributed as dist
    from adaface_amd.parallel import init_distributed, launch_ranks, launched_by_torchrun
    if opt.gpus > 1 and not launched_by_torchrun():   # before this process touches the GPU
        raise SystemExit(launch_ranks(opt.gpus, os.fspath(Path(__file__).resolve()), sys.argv[1:]))
    local = int(os.environ.get("LOCAL_RANK", "0")) if opt.gpu is None else opt.gpu
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: adaface_amd has no CPU path (use the reference for CPU plumbing runs)")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    rank, world = init_distributed(opt.gpus, backend="nccl", device=device)   # fails if the group is not opt.gpus ranks
    from adaface_amd.configs import sd15_config
    from adaface_amd.parallel import gather_frames, shard_batch, shard_range
    from adaface_amd.synth import synth_context
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.util import instantiate_from_config, load_config, load_model_from_config

    config = load_config(opt.config) if opt.config else sd15_config()
    from adaface_amd import img2img as I2I
    hybrid = I2I.select_hybrid(config, opt.ckpt)     # a 9-channel U-Net in the config or the checkpoint: the inpainting model
    problem = hybrid_problem(opt, hybrid)
    if problem:
        raise SystemExit(problem)
    if opt.ckpt:
        model = load_model_from_config(config, opt.ckpt)
    else:
        model = instantiate_from_config(config["model"]).eval()
    model = model.to(device)
    model = model.set_compute_dtype(opt.dtype, fp8_scope=opt.fp8_scope) if opt.dtype == "fp8" else model.set_compute_dtype(opt.dtype)
    if opt.tome > 0.0:
        model.set_token_merging(opt.tome, opt.tome_max_downsample)
    if opt.freeu is not None:
        model.set_freeu(opt.freeu_version, *opt.freeu)
    if opt.pag_scale > 0.0:
        model.set_pag(opt.pag_layers)
    if not opt.ckpt:  # seeded synthetic weights (identical on every rank)
        g = torch.Generator(device=device).manual_seed(1234)
        with torch.no_grad():
            for name, p in sorted(model.named_parameters()):
                if p.dim() == 1:
                    t = torch.randn(p.shape, generator=g, device=device)
                    p.copy_(1.0 + 0.1 * t if name.endswith(".weight") else 0.05 * t)
                else:
                    p.copy_(torch.randn(p.shape, generator=g, device=device) * p[0].numel() ** -0.5)
        model.model.diffusion_model._mark_dirty()
        model.first_stage_model._mark_dirty()
    if opt.lora:   # before any conditioning is made: a text-tower adapter changes the context; the same set on every rank
        from adaface_amd.lora import load_lora_file, split_lora
        unet = model.model.diffusion_model
        adapters = []
        for path, scale in opt.lora:
            split = split_lora(load_lora_file(path), unet._layout_kwargs(), strict=opt.lora_strict)
            if split["unused"] and rank == 0:
                print(f"--lora {path}: {len(split['unused'])} keys map onto no layer and are ignored, e.g. {split['unused'][:3]}")
            adapters.append((split, scale))
        model.set_lora(adapters)
        if rank == 0:
            print(f"--lora: {len(adapters)} adapter(s) on {len(unet.lora_targets())} U-Net weights")

    B = opt.n_samples
    lo, hi = shard_range(B, rank, world)
    b = hi - lo
    if opt.controlnet:   # identity from the model, pose from the ControlNet: its own engine, bf16 beside an fp8 U-Net
        from adaface_amd import layout
        from adaface_amd.ldm.modules.diffusionmodules.controlnet import SD15_CONTROLNET, ControlNet
        from adaface_amd.synth import synth_controlnet_state_dict, synth_hint
        unet = model.model.diffusion_model
        path, scale = opt.controlnet
        ctor = {**SD15_CONTROLNET, **{k: v for k, v in unet._layout_kwargs().items() if k != "out_channels"}, "num_heads": unet.num_heads}
        if path == "synthetic":
            cnet = ControlNet(**ctor)
            cnet.load_control_state_dict(synth_controlnet_state_dict(layout.controlnet_param_shapes(**cnet._layout_kwargs()), seed=4321))
        else:
            cnet = ControlNet.from_file(path, **{k: v for k, v in ctor.items() if k not in SD15_CONTROLNET or SD15_CONTROLNET[k] != v})
        cnet = cnet.to(device).set_compute_dtype("bf16" if opt.dtype == "fp8" else opt.dtype)
        if opt.control_image:
            hints = torch.cat([load_hint(p, opt.H, opt.W) for p in opt.control_image])
        else:
            hints = synth_hint(1, opt.seed + 4, opt.H, opt.W)
        hint = hints if hints.shape[0] == 1 else hints[lo:hi]      # (one per GLOBAL sample index: this rank's)
        unet.set_control(cnet, hint.to(device), scale=scale, t_range=opt.control_t_range, cond_only=opt.control_cond_only)
        if rank == 0:
            print(f"--controlnet: {path} x {scale:g}, timesteps {opt.control_t_range[0]} .. {opt.control_t_range[1]}"
                  f"{', conditional leg only' if opt.control_cond_only else ''}")
    if opt.prompt_emb:
        c_all = load_emb(opt.prompt_emb, B, "cpu")
        uc_all = load_emb(opt.neg_prompt_emb, B, "cpu") if opt.neg_prompt_emb else torch.zeros_like(c_all)
    elif opt.synthetic:
        c_all = synth_context(B, seed=opt.seed + 1, device="cpu")
        uc_all = synth_context(B, seed=opt.seed + 2, device="cpu", shared=True)
    else:
        raise SystemExit("give --prompt_emb (pre-computed CLIP/AdaFace embedding) or --synthetic")
    if opt.region_n:
        # regional prompts: the context becomes [base | region 1 | ...] along the token axis (the negative prompt repeated for
        # the unconditional legs) and the weight map of this rank's samples goes to the U-Net
        from adaface_amd import regions as RG
        Hl, Wl = opt.H // opt.f, opt.W // opt.f
        n = opt.region_n
        if opt.regions is not None:
            embs = [synth_context(B, seed=opt.seed + 10 + i, device="cpu") for i in range(n)]
            masks = RG.masks_from_boxes([(i / n, 0.0, (i + 1) / n, 1.0, 1.0) for i in range(n)], Hl, Wl)
        else:
            embs = [load_emb(p, B, "cpu") for p in opt.region_emb]
            masks = (RG.masks_from_boxes(opt.region_box, Hl, Wl) if opt.region_box
                     else torch.stack([RG.mask_from_image(p, Hl, Wl) for p in opt.region_mask]))
        both = RG.concat_contexts([c_all] + embs, uc_all)
        c_all, uc_all = both[: c_all.shape[0]].contiguous(), both[c_all.shape[0]:].contiguous()
        model.set_regions(RG.build_weights(masks, opt.region_base_weight, b, 2))
        if rank == 0:
            print(f"regional prompts: {n} region(s) + the base prompt at weight {opt.region_base_weight:g}, {c_all.shape[1]} keys per sample")
    c = model.get_learned_conditioning(shard_batch(c_all, rank, world, per_sample=16).to(device))
    uc = model.get_learned_conditioning(shard_batch(uc_all, rank, world, per_sample=16).to(device))
    i2i = {}
    x0 = keep = None
    if opt.img2img:
        # this rank's images and masks, by GLOBAL sample index.  Before the fp8 calibration: its sample runs the model, and a
        # hybrid model needs its concatenated condition for that
        imgs = I2I.load_batch(opt.img2img, B, lo, hi, opt.H, opt.W, I2I.load_image, "--img2img").to(device)
        x0 = I2I.encode_image(model, imgs)
        i2i = dict(x0=x0, strength=opt.strength, fused_blend=True)
        if opt.inpaint_mask:
            repaint = I2I.load_batch(opt.inpaint_mask, B, lo, hi, opt.H, opt.W, I2I.load_mask, "--inpaint_mask").to(device)
            keep = I2I.repaint_to_keep(repaint, opt.f)
            i2i["mask"] = keep
            if hybrid:
                model.set_concat_cond(I2I.concat_cond(model, imgs, repaint, opt.f))
        if rank == 0:
            print(f"--img2img: strength {opt.strength:g}" + (f", inpainting ({float(1.0 - keep.mean()):.0%} of this rank's latent "
                  f"cells repainted{', hybrid U-Net' if hybrid else ''})" if keep is not None else ""))
    if opt.dtype == "fp8":
        # static activation scales: from the file when it exists, else from a short calibration sample with this run's
        # conditioning.  With several ranks and a file to write, rank 0 calibrates on its shard and the others load what it
        # wrote; without a file every rank calibrates on its own shard
        def calibrate():
            lat = [opt.C, opt.H // opt.f, opt.W // opt.f]
            x_cal = torch.randn([b] + lat, generator=torch.Generator().manual_seed(opt.seed + 3))
            cal = model.calibrate_fp8(c, uc, shape=lat, batch_size=b, S=opt.fp8_calib_steps,
                                      guidance_scale=opt.scale if len(opt.scale) > 1 else opt.scale[0], x_T=x_cal.to(device))
            shifts = sorted(set(s for _, s, _ in cal.values()))
            print(f"[rank {rank}] fp8 calibration: {len(cal)} sites, shifts {shifts[0]} .. {shifts[-1]}, largest |activation| "
                  f"{max(a for a, _, _ in cal.values()):.1f}, {sum(k for _, _, k in cal.values())} elements saturated in the last pass")
            if opt.fp8_scales:
                model.save_fp8_scales(opt.fp8_scales)

        def agreed(flag):     # rank 0's answer on every rank (each rank looking for itself could disagree while rank 0 writes)
            if world == 1:
                return bool(flag)
            t = torch.tensor([int(bool(flag))], device=device)
            dist.broadcast(t, 0)
            return bool(t.item())

        if agreed(bool(opt.fp8_scales) and os.path.exists(opt.fp8_scales)):
            model.load_fp8_scales(opt.fp8_scales)
        elif opt.fp8_calib_steps > 0:
            if opt.fp8_scales and world > 1:
                err = None
                if rank == 0:
                    try:
                        calibrate()
                    except Exception as e:      # the others wait in the broadcast below: tell them before leaving
                        err = e
                if not agreed(err is None):
                    raise SystemExit(f"[rank {rank}] fp8 calibration failed on rank 0" + (f": {err!r}" if err is not None else ""))
                if rank != 0:
                    model.load_fp8_scales(opt.fp8_scales)
            else:
                calibrate()
    if opt.plms:
        from ldm.models.diffusion.plms import PLMSSampler
        sampler = PLMSSampler(model)
    elif opt.dpm_solver:
        from ldm.models.diffusion.dpm_solver import DPMSolverSampler
        sampler = DPMSolverSampler(model)
    elif opt.lcm:
        from ldm.models.diffusion.lcm import LCMSampler
        if opt.lcm_guidance_embedding and not model.has_guidance_embedding:
            raise SystemExit("--lcm_guidance_embedding: this model has no guidance-scale embedding (a --config whose unet_config "
                             "sets time_cond_proj_dim, and a checkpoint with time_embed.cond_proj.weight, are needed)")
        sampler = LCMSampler(model)
    else:
        sampler = DDIMSampler(model)
    shape = [opt.C, opt.H // opt.f, opt.W // opt.f]
    gs = opt.scale if len(opt.scale) > 1 else opt.scale[0]
    gen = torch.Generator().manual_seed(opt.seed)  # host RNG: the start code does not depend on the world size
    start_code = torch.randn([B] + shape, generator=gen) if opt.fixed_code else None
    noise_source = None
    if opt.noise == "philox":
        # this rank's samples carry their GLOBAL indices lo .. hi - 1: their noise does not depend on the world size
        from adaface_amd.noise import STREAM_XT, PhiloxNoise
        noise_source = PhiloxNoise(opt.seed, first_id=lo)
    if opt.init_img_paths:
        # stable_txt2img.py:594-625: encode each init image, average (divide by sqrt(N)), blend with noise
        avg = torch.zeros([B] + shape)
        for path in opt.init_img_paths:
            img = load_img(path, opt.H, opt.W).repeat(b, 1, 1, 1).to(device)
            enc = model.get_first_stage_encoding(model.encode_first_stage(img))   # this rank's samples
            avg[lo:hi] += enc.cpu()
        if world > 1:
            dist.all_reduce(avg_dev := avg.to(device))
            avg = avg_dev.cpu()
        avg /= np.sqrt(len(opt.init_img_paths))
        start_code = avg * opt.init_img_weight
        if noise_source is None:
            start_code = start_code + torch.randn([B] + shape, generator=gen) * (1.0 - opt.init_img_weight)
    hires_code = None
    if opt.hires is not None:
        from adaface_amd import hires as HR
        from adaface_amd.noise import STREAM_XT
        if rank == 0:
            print(f"hires fix: {opt.H}x{opt.W} -> {opt.hires[0] * opt.f}x{opt.hires[1] * opt.f}, upscaler {opt.hires_upscaler}, "
                  f"strength {opt.hires_strength:g}, {opt.hires_steps or opt.ddim_steps} steps")
    os.makedirs(opt.outdir, exist_ok=True)
    tic = time.time()
    count = 0
    with torch.no_grad(), model.ema_scope():
        for n in range(opt.n_repeat):
            if noise_source is None:
                x_T_all = start_code if start_code is not None else torch.randn([B] + shape, generator=gen)
                x_T = shard_batch(x_T_all, rank, world).to(device)
            else:
                # stream 0; step = the repeat index, or 0 for every repeat under --fixed_code
                x_T = noise_source.randn([b] + shape, STREAM_XT, 0 if opt.fixed_code else n, device)
                if opt.init_img_paths:
                    x_T = shard_batch(start_code, rank, world).to(device) + x_T * (1.0 - opt.init_img_weight)
            kw = {} if noise_source is None else dict(noise_source=noise_source)
            guided = {}
            if opt.pag_scale > 0.0 or opt.guidance_rescale > 0.0:
                guided = dict(pag_scale=opt.pag_scale, pag_adaptive_scale=opt.pag_adaptive_scale, guidance_rescale=opt.guidance_rescale)
            if opt.sag_scale > 0.0:
                guided = dict(sag_scale=opt.sag_scale, sag_blur_sigma=opt.sag_blur_sigma)
            kw.update(guided)
            if opt.deep_cache not in (None, 1):
                kw.update(deep_cache_interval=opt.deep_cache, deep_cache_depth=opt.deep_cache_depth)
            if opt.tgate:
                kw.update(tgate_step=opt.tgate)
            kw.update(i2i)        # (--img2img: x_T is then the noise added to x0, not a latent)
            guided.update(i2i)
            if opt.plms:
                call = dict(S=opt.ddim_steps, conditioning=c, batch_size=b, shape=shape, verbose=False,
                            unconditional_guidance_scale=opt.scale[0], unconditional_conditioning=uc,
                            eta=opt.ddim_eta, x_T=x_T, **guided)
            elif opt.dpm_solver:
                call = dict(S=opt.ddim_steps, conditioning=c, batch_size=b, shape=shape, verbose=False,
                            guidance_scale=gs, unconditional_conditioning=uc, eta=opt.ddim_eta, x_T=x_T,
                            skip_type=opt.dpm_skip, algorithm="sde-dpmsolver++" if opt.dpm_sde else "dpmsolver++",
                            **kw)
            elif opt.lcm:
                call = dict(S=opt.ddim_steps, conditioning=c, batch_size=b, shape=shape, verbose=False,
                            guidance_scale=gs, unconditional_conditioning=uc, x_T=x_T,
                            original_steps=opt.lcm_original_steps, tcd_gamma=opt.tcd_gamma,
                            guidance_embedding=opt.lcm_guidance_embedding, **kw)
            else:
                call = dict(S=opt.ddim_steps, conditioning=c, batch_size=b, shape=shape, verbose=False,
                            guidance_scale=gs, unconditional_conditioning=uc, eta=opt.ddim_eta, x_T=x_T, **kw)
            if opt.hires is None:
                samples, _ = sampler.sample(**call)
            else:
                # pass two: the same sampler, guidance and opt-ins on the upscaled result; its noise from the derived Philox
                # source, or from the host generator the start code came from (the same for every world size)
                second = HR.second_kwargs(call, steps=opt.hires_steps)
                shape2 = [opt.C, *opt.hires]
                if noise_source is None:
                    if hires_code is None or not opt.fixed_code:
                        hires_code = torch.randn([B] + shape2, generator=gen)
                    z2 = shard_batch(hires_code, rank, world).to(device)
                else:
                    z2 = second["noise_source"].randn([b] + shape2, STREAM_XT, 0 if opt.fixed_code else n, device)
                samples, _ = HR.two_pass(sampler, call, second, opt.hires, opt.hires_upscaler, opt.hires_strength, noise=z2)
            if keep is not None:      # the kept region is the image's own encoding, without the last blend's noise
                samples = I2I.finish(samples, x0, keep)
            frames = gather_frames(model.decode_first_stage_uint8(samples), global_batch=B)
            if rank == 0 and not opt.skip_save:
                from PIL import Image
                for i, f in enumerate(frames.cpu().numpy()):
                    Image.fromarray(f).save(os.path.join(opt.outdir, f"{count:05}.jpg"))
                    count += 1
    torch.cuda.synchronize()
    toc = time.time()
    if rank == 0:
        n_img = B * opt.n_repeat
        out_h, out_w = (opt.H, opt.W) if opt.hires is None else (opt.hires[0] * opt.f, opt.hires[1] * opt.f)
        print(f"{n_img} images of {out_h}x{out_w} @ {opt.ddim_steps} {'PLMS' if opt.plms else 'DPM-Solver++(2M) SDE' if opt.dpm_sde else 'DPM-Solver++(2M)' if opt.dpm_solver else 'TCD' if opt.tcd_gamma is not None else 'LCM' if opt.lcm else 'DDIM'} steps in {toc - tic:.2f} s "
              f"({n_img / (toc - tic):.2f} images/s incl. first-call warm-up) on {world} GPU(s); outputs: {opt.outdir}")
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
