"""The MotionClone guidance layer with the reference's function names and signatures
(reference motionclone/utils/motionclone_functions.py), to be bound onto pipeline / scheduler / unet with
`fn.__get__(obj)` exactly as t2v_video_sample.py:57-65 does.  Arithmetic runs in the HIP engine
(motionclone_amd/engine.py); these functions only orchestrate and keep the reference's quirks:
CFG is eps_c + s (eps_c - eps_u) (:239,255); extraction uses the empty-prompt embedding at add_noise_step (:36-41);
warm-up / cool-down factors (:228-234); x0 of the DDIM update uses the un-guided eps (:340,375-389)."""
import os  # noqa: F401  (re-exported: the reference's entry scripts rely on `import *` providing these names)
from dataclasses import dataclass
from typing import Optional

import numpy as np  # noqa: F401
import torch

from .. import ops
from ..engine import MAX_TOPK
from ..sampler import MotionCloneSampler, uneven_timesteps
from .conv_layer import prep_unet_conv  # noqa: F401
from .util import classify_blocks, set_all_seed, video_preprocess  # noqa: F401
from .xformer_attention import MySelfAttnProcessor, prep_unet_attention  # noqa: F401

try:  # einops / imageio are re-exported by the reference module; keep the names when available
    from einops import rearrange  # noqa: F401
except ImportError:  # pragma: no cover
    rearrange = None
try:
    import imageio  # noqa: F401
except ImportError:  # pragma: no cover
    imageio = None


@dataclass
class UNet3DConditionOutput:
    sample: torch.Tensor


def add_noise(self, timestep, x_0, noise_pred):
    """:19-23"""
    alpha_prod_t = self.scheduler.alphas_cumprod[timestep]
    beta_prod_t = 1 - alpha_prod_t
    return (alpha_prod_t ** 0.5 * x_0.float() + beta_prod_t ** 0.5 * noise_pred.float()).to(x_0.dtype)


def _sampler(pipe):
    """MotionCloneSampler over the pipeline's unet engine.  Hyper-parameters come from pipe.input_config; the timestep
    table, alphas_cumprod and final_alpha_cumprod are READ FROM pipe.scheduler, as the reference does (:213-214,326-336),
    so any spacing type / beta schedule / set_alpha_to_one the scheduler was configured with is honoured.  Cached.
    On the GPU every DDIM step is captured into a hipGraph at its first use and replayed for every later video of the same
    shape (sampler.enable_graphs; bit-identical to the eager launch sequence, which eta > 0 and MC_NO_GRAPHS=1 still take):
    the reference API runs the same path bench.py times."""
    c = pipe.input_config
    sch = pipe.scheduler
    # reading the scheduler's tables is a device -> host copy: done again only when the scheduler's tensors were replaced or
    # written (customized_set_timesteps assigns a new tensor), not on every step.  The cache HOLDS the tensor objects and
    # compares with `is` + `_version` (an id() alone can be reused by a new tensor once the old one is freed); tables that are
    # not tensors (numpy arrays, lists: in-place edits leave no trace) are re-read every call - they are host data anyway.
    cached = getattr(pipe, "_mc_sched_src", None)
    fresh = (cached is None or cached[0] is not sch.timesteps or cached[2] is not sch.alphas_cumprod
             or not isinstance(sch.timesteps, torch.Tensor) or not isinstance(sch.alphas_cumprod, torch.Tensor)
             or cached[1] != sch.timesteps._version or cached[3] != sch.alphas_cumprod._version)
    if fresh:
        pipe._mc_sched_tables = (tuple(int(t) for t in torch.as_tensor(sch.timesteps).cpu().tolist()),
                                 torch.as_tensor(sch.alphas_cumprod).detach().float().cpu())
        pipe._mc_sched_src = (sch.timesteps, getattr(sch.timesteps, "_version", 0), sch.alphas_cumprod,
                              getattr(sch.alphas_cumprod, "_version", 0))
    ts, acp = pipe._mc_sched_tables
    final = float(getattr(sch, "final_alpha_cumprod", 1.0))
    if len(ts) != int(c.inference_steps):
        raise ValueError("scheduler holds %d timesteps but input_config.inference_steps = %d: run "
                         "scheduler.customized_set_timesteps first" % (len(ts), int(c.inference_steps)))
    key = (id(pipe.unet.engine()), c.cfg_scale, c.motion_guidance_weight, c.warm_up_steps, c.cool_up_steps,
           c.inference_steps, c.guidance_steps, c.guidance_scale, ts, hash(acp.numpy().tobytes()), final)
    if getattr(pipe, "_mc_sampler_key", None) != key:
        pipe._mc_sampler = MotionCloneSampler(pipe.unet.engine(), cfg_scale=c.cfg_scale,
                                              motion_guidance_weight=c.motion_guidance_weight,
                                              warm_up_steps=c.warm_up_steps, cool_up_steps=c.cool_up_steps,
                                              num_inference_steps=c.inference_steps, guidance_steps=c.guidance_steps,
                                              guidance_scale=c.guidance_scale, timesteps=ts, alphas_cumprod=acp,
                                              final_alpha_cumprod=final)
        if pipe._mc_sampler.dev.type == "cuda" and os.environ.get("MC_NO_GRAPHS", "0") != "1":
            pipe._mc_sampler.enable_graphs()
        pipe._mc_sampler_key = key
    return pipe._mc_sampler


def _motion_topk(cfg, override=None):
    """sparsity k of the motion representation to EXTRACT: the optional inference-yaml key `motion_topk` (absent: 1, the
    reference's torch.topk(k=1) of :79) or a per-call override.  Sampling never reads it: the steps take k from the
    representation they are given."""
    k = override if override is not None else getattr(cfg, "motion_topk", None)
    return 1 if k is None else int(k)


def _load_mask(m):
    """a motion mask given as a tensor / array or as the path of a `.pt` (torch.save of the tensor) or `.npy` file"""
    if m is None or isinstance(m, torch.Tensor):
        return m
    if isinstance(m, (str, os.PathLike)):
        path = os.fspath(m)
        if path.endswith(".npy"):
            return torch.from_numpy(np.load(path))
        if path.endswith(".pt"):
            return torch.as_tensor(torch.load(path, map_location="cpu"))
        raise ValueError("motion mask file %s: expected a .pt or .npy file" % path)
    return torch.as_tensor(m)


def _motion_mask(pipe, override=None):
    """the motion mask of the next sampling run (where the reference motion is cloned; engine.check_motion_mask): a per-call /
    per-example override (tensor or path), else the pipeline attribute `motion_mask`, else the optional inference-yaml key
    `motion_mask_path`; None = no mask, every path as without the feature.  -> (tensor or None, motion_mask_normalize)"""
    cfg = pipe.input_config
    m = override
    if m is None:
        m = getattr(pipe, "motion_mask", None)
    if m is None:
        m = getattr(cfg, "motion_mask_path", None)
    return _load_mask(m), bool(getattr(cfg, "motion_mask_normalize", False) or False)


_REFERENCE_KEYS = ("representation_path", "representation", "weight", "mask_path", "mask", "mask_normalize")


def _motion_references(pipe, override=None):
    """further motion references of the next sampling run (motion composition; engine.prepare_representation `references`): a
    per-call / per-example override, else the `motion_references` key of the examples-file line a launcher thread is working
    on, else the pipeline attribute `motion_references`, else the optional inference-yaml key `motion_references` - a list of
    {representation_path: x.pt (a file written by obtain_motion_representation, any motion_topk) or representation: the
    loaded dict, weight: 1.0, mask_path: m.pt | m.npy (or mask: a tensor), mask_normalize: false}.  None / empty = no further
    reference, every path as without the feature.  The example's own reference keeps `motion_mask_path`."""
    from .. import lanes
    from ..checkpoints import _real_torch_load
    refs = override
    if refs is None:
        refs = lanes.example().get("motion_references")
    if refs is None:
        refs = getattr(pipe, "motion_references", None)
    if refs is None:
        refs = getattr(pipe.input_config, "motion_references", None)
    if refs is None or len(refs) == 0:
        return None
    out = []
    for r, ref in enumerate(refs, 1):
        if isinstance(ref, (str, bytes)) or not hasattr(ref, "keys"):
            raise ValueError("motion_references entry %d: a mapping {representation_path, weight, mask_path, mask_normalize} is "
                             "expected, got %r" % (r, ref))
        ref = {k: ref[k] for k in ref.keys()}
        unknown = sorted(set(ref) - set(_REFERENCE_KEYS))
        if unknown:
            raise ValueError("motion_references entry %d: unknown keys %s (known: %s)" % (r, unknown, list(_REFERENCE_KEYS)))
        rep = ref.get("representation")
        if rep is None:
            path = ref.get("representation_path")
            if path is None:
                raise ValueError("motion_references entry %d: representation_path (or representation) is missing" % r)
            rep = _real_torch_load(os.fspath(path), map_location="cpu")     # the per-example file, read by the thread that uses it
        mask = ref.get("mask")
        w = ref.get("weight")
        out.append(dict(representation=rep, weight=1.0 if w is None else float(w),
                        mask=_load_mask(mask if mask is not None else ref.get("mask_path")),
                        mask_normalize=bool(ref.get("mask_normalize") or False)))
    return out


def _context(cfg, frames):
    """Sliding context windows of a long video (sampler.MotionCloneSampler.windows): the optional inference-yaml keys
    `context_length` (L <= 32), `context_overlap` (default L // 4) and `context_weights` ('triangular', the default, or
    'uniform').  -> (the sampler's `context` dict, the windows' first frames), or (None, []) when `context_length` is absent or
    the `frames` of the run fit one window: every path is then as without the keys.  `video_length` may exceed 32 with them."""
    L = getattr(cfg, "context_length", None)
    if L is None:
        for k in ("context_overlap", "context_weights"):
            if getattr(cfg, k, None) is not None:
                raise ValueError("%s is set without context_length" % k)
        return None, []
    L = int(L)
    ov = getattr(cfg, "context_overlap", None)
    ctx = dict(length=L, overlap=L // 4 if ov is None else int(ov), weights=getattr(cfg, "context_weights", None) or "triangular")
    if ctx["weights"] not in ops.CONTEXT_WEIGHTS:
        raise ValueError("context_weights: %r, expected one of %s" % (ctx["weights"], list(ops.CONTEXT_WEIGHTS)))
    starts = ops.context_windows(frames, L, ctx["overlap"])
    return (ctx, starts) if starts else (None, [])


def _window_representations(rep, ctx, frames, nW):
    """a representation written by obtain_motion_representation under a context ({module: [values, indices]} with the windows
    folded window-major into the row axis, plus "motion_context") -> the list of the nW windows' representations; a file that
    was extracted for another video length / context, or without one, is refused"""
    want = dict(frames=int(frames), length=ctx["length"], overlap=ctx["overlap"])
    mc = rep.get("motion_context") if hasattr(rep, "get") else None
    if mc is None:
        raise ValueError("context_length: the motion representation carries no motion_context entry - it was extracted without "
                         "context windows; the run needs %s (run obtain_motion_representation with the same yaml keys)" % want)
    have = {k: int(mc[k]) for k in ("frames", "length", "overlap") if k in mc}
    if have != want:
        raise ValueError("context_length: the motion representation was extracted with motion_context %s, the run has %s"
                         % (have, want))
    out = [dict() for _ in range(nW)]
    for name, ent in rep.items():
        if name == "motion_context":
            continue
        val, idx = ent[0], ent[1]
        if val.shape[0] % nW:
            raise ValueError("context_length: motion representation %s has %d rows, no multiple of the %d windows"
                             % (name, val.shape[0], nW))
        n = val.shape[0] // nW
        for w in range(nW):
            out[w][name] = [val[w * n:(w + 1) * n], idx[w * n:(w + 1) * n]]
    return out


@torch.no_grad()
def obtain_motion_representation(self, generator=None, motion_representation_path: str = None, duration=None,
                                 use_controlnet=False, video_latents=None, uncond_embeddings=None, video_data=None,
                                 motion_topk=None):
    """:25-82.  `video_latents` / `uncond_embeddings` let synthetic inputs bypass decord / VAE / CLIP (`video_data`
    [F, 3, H, W] in [-1, 1]: the preprocessed frames, needed beside `video_latents` only by the pixel-condition ControlNet).
    `motion_topk` (default: input_config.motion_topk, absent = 1): top-k values / indices per attention row, saved in the
    reference's layout with last dimension k.
    With the yaml key `context_length` and a reference longer than it (`_context`): one noise tensor for the long latent, the
    windows of the noisy latent run as one batch; the entries hold the windows folded window-major into the row axis
    ([nW BN, heads, L, k]) and an entry "motion_context": {frames, length, overlap} names what they were extracted for."""
    cfg = self.input_config
    topk = _motion_topk(cfg, motion_topk)
    if video_latents is None:
        if video_data is None:
            video_data = video_preprocess(cfg.video_path, cfg.height, cfg.width, cfg.video_length, duration=duration)
        lat = self.vae.encode(video_data.to(self.vae.dtype).to(self.vae.device)).latent_dist.sample(None)
        video_latents = (self.vae.config.scaling_factor * lat).unsqueeze(0).permute(0, 2, 1, 3, 4).contiguous()
    if uncond_embeddings is None:
        tok = self.tokenizer([""], padding="max_length", max_length=self.tokenizer.model_max_length, return_tensors="pt")
        uncond_embeddings = self.text_encoder(tok.input_ids.to(self.device))[0]
    step_t = int(cfg.add_noise_step)
    noise = torch.randn(video_latents.shape, generator=generator, device=video_latents.device, dtype=video_latents.dtype)
    noisy = self.add_noise(step_t, video_latents, noise)
    ctx, starts = _context(cfg, video_latents.shape[2])
    if starts:
        if use_controlnet:
            raise NotImplementedError("context_length: SparseCtrl (use_controlnet) with context windows is not supported")
        if video_latents.shape[0] != 1:
            raise ValueError("context_length: one long reference video [1, 4, F, H, W] is expected, got %s" % (tuple(video_latents.shape),))
        noisy = ops.latent_windows(noisy.half(), ctx["length"], ctx["overlap"])
        uncond_embeddings = uncond_embeddings[0:1].expand(len(starts), -1, -1)
    down_res = mid_res = None
    if use_controlnet:   # :46-72: condition = the reference video's own frames at image_index
        idx = cfg.image_index
        if self.controlnet.use_simplified_condition_embedding:       # :48-49 VAE latents
            src = video_latents
        else:                                                        # :50-52 pixels in [0, 1]
            if video_data is None:
                raise ValueError("the pixel-condition SparseCtrl needs the preprocessed frames (video_data)")
            src = ((video_data.unsqueeze(0).to(video_latents.device, video_latents.dtype).permute(0, 2, 1, 3, 4) + 1) / 2)
        cond = torch.zeros_like(src)
        mask = torch.zeros_like(src[:, :1])
        cond[:, :, idx] = src[:, :, idx]
        mask[:, :, idx] = 1
        down_res, mid_res = self.controlnet(noisy, step_t, encoder_hidden_states=uncond_embeddings, controlnet_cond=cond,
                                            conditioning_mask=mask, conditioning_scale=cfg.controlnet_scale,
                                            guess_mode=False, return_dict=False)
    # partial forward up to the guidance block; the hooked attentions record their q / k (:74-76)
    self.unet(noisy.half(), step_t, encoder_hidden_states=uncond_embeddings.half(), return_dict=False,
              only_motion_feature=True, down_block_additional_residuals=down_res, mid_block_additional_residual=mid_res)
    rep = {}
    for name, module in self.unet.named_modules():
        if "VersatileAttention" in type(module).__name__ and classify_blocks(cfg.motion_guidance_blocks, name):
            r = module.processor.key
            C, g = r["C"], r["geo"]
            if not 1 <= topk <= min(g.F, MAX_TOPK):
                raise ValueError("motion_topk = %d outside 1 .. min(F = %d, %d)" % (topk, g.F, MAX_TOPK))
            if topk == 1:
                val, idx = ops.tattn_top1(r["qkv"][:, :C], r["qkv"][:, C:2 * C], g.B, g.F, g.hw, module.heads, r["d"])
            else:
                val, idx = ops.tattn_topk(r["qkv"][:, :C], r["qkv"][:, C:2 * C], g.B, g.F, g.hw, module.heads, r["d"], topk)
            rep[name] = [val, idx]   # topk(k) value / uint8 index (:79 with k = motion_topk)
    meta = dict(motion_context=dict(frames=int(video_latents.shape[2]), length=ctx["length"], overlap=ctx["overlap"])) if starts else {}
    if motion_representation_path is not None:
        # the reference's on-disk format: {module name: [values fp16 [BN, heads, F, k], indices uint8 [...]]} (:79-81)
        torch.save(dict({k: [v.cpu(), i.cpu()] for k, (v, i) in rep.items()}, **meta), motion_representation_path)
    rep.update(meta)
    self.motion_representation_path = motion_representation_path
    self.motion_representation_dict = rep
    return rep


def get_temp_attn_prob(self, index_select=None):
    """:260-283: P = softmax(scale q k^T) [(b n), heads, F, F] for every hooked temporal attention.  `index_select`
    (a 0/1 flag per equal block of the (b n) axis, :267-271 - e.g. [0, 1] keeps the second batch element) picks rows of
    the result: the probabilities are computed per (b, pixel) anyway, the selection is data movement."""
    out = {}
    for name, module in self.unet.named_modules():
        if "VersatileAttention" in type(module).__name__ and classify_blocks(self.input_config.motion_guidance_blocks, name):
            r = module.processor.key
            C, g = r["C"], r["geo"]
            prob = ops.tattn_prob(r["qkv"][:, :C], r["qkv"][:, C:2 * C], g.B, g.F, g.hw, module.heads, r["d"])
            if index_select is not None:
                rows = prob.shape[0]
                if rows % len(index_select):
                    raise ValueError("index_select of length %d does not divide %d rows" % (len(index_select), rows))
                keep = torch.repeat_interleave(torch.tensor(index_select), repeats=rows // len(index_select)).bool()
                prob = prob[keep.to(prob.device)]
            out[name] = prob
    return out


def compute_temp_loss(self, temp_attn_prob_control_dict):
    """:85-100: sum over hooked modules of mse(gather(P, ref_idx), ref_val), evaluated by the fused HIP loss kernel
    on the recorded q / k of each module (the dict argument supplies the module names)."""
    total = None
    for name in temp_attn_prob_control_dict.keys():
        module = dict(self.unet.named_modules())[name]
        r = module.processor.key
        C, g = r["C"], r["geo"]
        val, idx = self.motion_representation_dict[name]
        dev = r["qkv"].device
        lm = ops.tattn_loss(r["qkv"][:, :C], r["qkv"][:, C:2 * C], idx.to(dev, torch.uint8).contiguous(),
                            val.to(dev, torch.float32).contiguous(), g.B, g.F, g.hw, module.heads, r["d"])
        total = lm if total is None else total + lm
    return total.reshape(())


def single_step_video(self, noisy_latents, step_index, step_t, extra_step_kwargs):
    """:173-257 (guided branch while step_index < guidance_steps, else one B=2 forward)"""
    smp = _sampler(self)
    if int(step_t) != int(smp.timesteps[step_index]):
        raise ValueError("step_t %d is not scheduler.timesteps[%d] = %d" % (int(step_t), step_index,
                                                                            int(smp.timesteps[step_index])))
    ctrl = None
    ctx, starts = _context(self.input_config, noisy_latents.shape[2])
    if starts and getattr(self, "add_controlnet", False):
        raise NotImplementedError("context_length: SparseCtrl (add_controlnet) with context windows is not supported")
    if getattr(self, "add_controlnet", False):   # :176-197: condition latents placed at image_index, mask = 1 there
        smp.controlnet = self.controlnet.engine()
        ci = self.controlnet_images.to(noisy_latents.device, torch.float16)
        shape = list(ci.shape)
        shape[2] = noisy_latents.shape[2]
        cond = torch.zeros(shape, device=ci.device, dtype=ci.dtype)
        mask = torch.zeros([shape[0], 1] + shape[2:], device=ci.device, dtype=ci.dtype)
        cond[:, :, self.input_config.image_index] = ci
        mask[:, :, self.input_config.image_index] = 1
        ctrl = dict(cond=cond, mask=mask, scale=self.input_config.controlnet_scale)
    if not hasattr(self, "_mc_mask"):            # called without sample_video: the configured mask, read once
        self._mc_mask = _motion_mask(self)
    mask, mask_norm = self._mc_mask
    if not hasattr(self, "_mc_refs"):            # called without sample_video: the configured further references, read once
        self._mc_refs = _motion_references(self)
    if (getattr(self, "_mc_rep_src", None) is not self.motion_representation_dict
            or getattr(self, "_mc_rep_mask", None) is not self._mc_mask
            or getattr(self, "_mc_rep_refs", None) is not self._mc_refs):
        if starts:                               # a long video: the windows' representations as one packed batch, once per video
            if self._mc_refs is not None:
                raise NotImplementedError("context_length: motion_references with context windows is not supported")
            F = noisy_latents.shape[2]
            self._mc_rep_dev = smp.prepare_windows(_window_representations(self.motion_representation_dict, ctx, F, len(starts)),
                                                   smp.windows(ctx, F), F, mask=mask, mask_normalize=mask_norm,
                                                   grid=tuple(noisy_latents.shape[3:]))
        elif "motion_context" in self.motion_representation_dict:
            raise ValueError("the motion representation was extracted with motion_context %s, but this run of %d frames has no "
                             "context windows (yaml key context_length)" % (dict(self.motion_representation_dict["motion_context"]),
                                                                            noisy_latents.shape[2]))
        elif self._mc_refs is not None:            # motion composition: merged with the example's own reference here, once per video
            self._mc_rep_dev = smp.engine.prepare_representation(self.motion_representation_dict, frames=noisy_latents.shape[2],
                                                                 mask=mask, mask_normalize=mask_norm,
                                                                 grid=tuple(noisy_latents.shape[3:]), references=self._mc_refs)
        elif mask is None:
            self._mc_rep_dev = smp.engine.prepare_representation(self.motion_representation_dict, frames=noisy_latents.shape[2])
        else:                                    # reduced to the hooked modules' grids here, once per video
            self._mc_rep_dev = smp.engine.prepare_representation(self.motion_representation_dict, frames=noisy_latents.shape[2],
                                                                 mask=mask, mask_normalize=mask_norm,
                                                                 grid=tuple(noisy_latents.shape[3:]))
        self._mc_rep_src = self.motion_representation_dict
        self._mc_rep_mask = self._mc_mask
        self._mc_rep_refs = self._mc_refs
    kw = dict(extra_step_kwargs or {})      # prepare_extra_step_kwargs: eta / generator, handed to customized_step (:241,255)
    out = smp.step(noisy_latents.half(), step_index, self.text_embeddings.half(), self._mc_rep_dev, ctrl=ctrl,
                   eta=float(kw.get("eta", 0.0) or 0.0), generator=kw.get("generator") if kw.get("eta") else None, context=ctx)
    # a replayed step returns the graph's STATIC output buffer (sampler._graphed_step), which the next replay of the same
    # step index - the next video - overwrites; the reference API hands out fresh tensors, so the boundary copies (0.5 MiB)
    if smp._graphs is not None:
        out = out.clone()
    return out.detach()


def sample_video(self, eta: float = 0.0, generator=None, noisy_latents: Optional[torch.Tensor] = None,
                 add_controlnet: bool = False, text_embeddings=None, decode=True, controlnet_images=None, motion_mask=None,
                 motion_references=None):
    """:102-171.  `motion_mask` (tensor or path; default: the pipeline attribute `motion_mask`, then the yaml key
    `motion_mask_path`): region weights of the guidance for this video.  `motion_references` (default: the examples-file
    line's, the pipeline attribute's, then the yaml key's `motion_references`): further motion references that guide this
    video beside its own (`_motion_references`)."""
    self.add_controlnet = add_controlnet
    cfg = self.input_config
    self._mc_mask = _motion_mask(self, motion_mask)
    self._mc_refs = _motion_references(self, motion_references)
    if add_controlnet and controlnet_images is not None:
        # already what the ControlNet consumes (:122-128): VAE latents [1, 4, n, h, w], or pixels in [0, 1] [1, 3, n, H, W]
        self.controlnet_images = controlnet_images
    elif add_controlnet:
        from PIL import Image
        import numpy as _np
        imgs = []
        for path in cfg.condition_image_path_list:       # :112-119 (Resize + ToTensor), then VAE encode (:121-126)
            im = Image.open(path).convert("RGB").resize((cfg.width, cfg.height), Image.BILINEAR)
            imgs.append(torch.from_numpy(_np.array(im)).permute(2, 0, 1).float() / 255.0)
        px = torch.stack(imgs).to(dtype=self.vae.dtype, device=self.vae.device)
        if self.controlnet.use_simplified_condition_embedding:       # :122-126
            lat = self.vae.encode(px * 2.0 - 1.0).latent_dist.sample() * self.vae.config.scaling_factor
            self.controlnet_images = lat.unsqueeze(0).permute(0, 2, 1, 3, 4).contiguous()
        else:                                                        # :127-128 pixel-space condition as it is
            self.controlnet_images = px.unsqueeze(0).permute(0, 2, 1, 3, 4).contiguous()
    device = self._execution_device
    if text_embeddings is None:
        text_embeddings = self._encode_prompt(cfg.new_prompt, device, 1, True, cfg.negative_prompt)
    self.text_embeddings = text_embeddings
    noisy_latents = self.prepare_latents(1, self.unet.config.in_channels, cfg.video_length, cfg.height, cfg.width,
                                         self.text_embeddings.dtype, device, generator, noisy_latents)
    if isinstance(getattr(self, "motion_representation_path", None), str) and os.path.exists(self.motion_representation_path):
        self.motion_representation_dict = torch.load(self.motion_representation_path)
    self.motion_scale = cfg.motion_guidance_weight
    from .. import lanes
    grp = lanes.group()
    if grp is not None and grp.size > 1 and _context(cfg, noisy_latents.shape[2])[1]:
        raise NotImplementedError("context_length: a launcher lane that packs several examples (--batch V > 1) with context "
                                  "windows is not supported; run with --batch 1")
    packed = _group_sample(self, grp, noisy_latents, eta, generator) if grp is not None and grp.size > 1 else None
    if packed is not None:     # the thread's lane carried this example through one packed launch sequence with its fellows'
        noisy_latents = packed
    else:
        extra_step_kwargs = self.prepare_extra_step_kwargs(generator, eta)
        with self.progress_bar(total=cfg.inference_steps) as progress_bar:
            for step_index, step_t in enumerate(self.scheduler.timesteps):
                noisy_latents = self.single_step_video(noisy_latents, step_index, step_t, extra_step_kwargs)
                progress_bar.update()
    if not decode:
        return noisy_latents
    return self.decode_latents(noisy_latents)


def _condition_images(pipe, ex):
    """what `sample_video` turns `controlnet_images` / `condition_image_path_list` into (:112-128) for one example"""
    cfg = pipe.input_config
    if ex.get("controlnet_images") is not None:
        return ex["controlnet_images"]
    from PIL import Image
    import numpy as _np
    imgs = []
    for path in ex.get("condition_image_path_list", getattr(cfg, "condition_image_path_list", None)):
        im = Image.open(path).convert("RGB").resize((cfg.width, cfg.height), Image.BILINEAR)
        imgs.append(torch.from_numpy(_np.array(im)).permute(2, 0, 1).float() / 255.0)
    px = torch.stack(imgs).to(dtype=pipe.vae.dtype, device=pipe.vae.device)
    if pipe.controlnet.use_simplified_condition_embedding:
        lat = pipe.vae.encode(px * 2.0 - 1.0).latent_dist.sample() * pipe.vae.config.scaling_factor
        return lat.unsqueeze(0).permute(0, 2, 1, 3, 4).contiguous()
    return px.unsqueeze(0).permute(0, 2, 1, 3, 4).contiguous()


def _placed(src, idx, frames=None):
    """condition tensor + mask with `src`'s frames at image_index `idx` (:46-72,176-197); src already holds `frames` frames
    (the reference video itself) or only the condition frames"""
    shape = list(src.shape)
    if frames is not None:
        shape[2] = frames
    cond = torch.zeros(shape, device=src.device, dtype=src.dtype)
    mask = torch.zeros([shape[0], 1] + shape[2:], device=src.device, dtype=src.dtype)
    cond[:, :, idx] = src[:, :, idx] if frames is None else src
    mask[:, :, idx] = 1
    return cond, mask


_MIXED = "either every example carries a condition image or none does"


@torch.no_grad()
def _packed_sample(self, latents, texts, reps, ctrls, eta=0.0, generators=None, masks=None, references=None):
    """The packed step loop on this pipeline's sampler for V videos whose per-example host work is done: `latents` V tensors
    [1, 4, F, H, W], `texts` V [2, n, dim] ([uncond, cond]), `reps` V motion representations, `ctrls` V SparseCtrl dicts
    (cond / mask [1, ...] placed at image_index, scale) or V times None, `generators` the V generators that `eta > 0` draws each
    video's variance noise from, in list order at every step, `masks` V motion masks (tensors or None; None = no mask at all),
    `references` V lists of further motion references (`_motion_references`) or None (None = none at all).
    Returns the final latents [V, 4, F, H, W] - after a replayed
    step the graph's static buffer: callers that keep them copy."""
    from ..sampler import batch_ctrl
    cfg = self.input_config
    V = len(latents)
    use_ctrl = [c is not None for c in ctrls]
    if any(use_ctrl) != all(use_ctrl):
        raise ValueError("sample_video_batch: " + _MIXED)
    smp = _sampler(self)
    ctrl = None
    if use_ctrl[0]:
        smp.controlnet = self.controlnet.engine()
        ctrl = batch_ctrl(list(ctrls), V)
    if references is not None and any(r is not None for r in references):
        rep_dev = smp.engine.prepare_representation(list(reps), frames=latents[0].shape[2],
                                                    mask=list(masks) if masks is not None else None,
                                                    mask_normalize=_motion_mask(self)[1], grid=tuple(latents[0].shape[3:]),
                                                    references=list(references))
    elif masks is None or all(m is None for m in masks):
        rep_dev = smp.engine.prepare_representation(list(reps), frames=latents[0].shape[2])   # one top-k K for the V videos
    else:
        rep_dev = smp.engine.prepare_representation(list(reps), frames=latents[0].shape[2], mask=list(masks),
                                                    mask_normalize=_motion_mask(self)[1], grid=tuple(latents[0].shape[3:]))
    x = torch.cat(list(latents), 0).half()
    text2 = torch.cat([t[0:1] for t in texts] + [t[1:2] for t in texts], 0).half()
    with self.progress_bar(total=cfg.inference_steps) as progress_bar:
        for i in range(len(smp.timesteps)):
            if eta:
                z = []
                for v in range(V):
                    gen = generators[v] if generators is not None else None
                    gdev = gen.device if gen is not None else x.device
                    z.append(torch.randn(x[v:v + 1].shape, generator=gen, device=gdev, dtype=x.dtype).to(x.device))
                x = smp.step(x, i, text2, rep_dev, ctrl=ctrl, eta=float(eta), variance_noise=torch.cat(z, 0))
            else:
                x = smp.step(x, i, text2, rep_dev, ctrl=ctrl)
            progress_bar.update()
    return x.detach()


def _run_group(grp, items):
    """the leader's part of the meeting point: the live members' examples through ONE packed launch sequence on the leader's
    pipeline, in the lane's stream; every member gets (a copy of its [1, 4, F, H, W] slice, the event that marks it complete).
    A lone member gets None: it runs the one-video loop itself."""
    if len(items) == 1:
        return [None]
    etas = {it["eta"] for it in items}
    if len(etas) != 1:
        raise ValueError("the examples of one packed group share one eta, got %s" % sorted(etas))
    pipe = items[0]["pipe"]
    on_gpu = items[0]["latents"].is_cuda

    def run():
        x = _packed_sample(pipe, [it["latents"] for it in items], [it["text"] for it in items], [it["rep"] for it in items],
                           [it["ctrl"] for it in items], eta=etas.pop(), generators=[it["generator"] for it in items],
                           masks=[it.get("mask") for it in items], references=[it.get("references") for it in items])
        return [x[v:v + 1].clone() for v in range(len(items))]
    if not on_gpu:
        return [(o, None) for o in run()]
    if grp.stream is None:
        grp.stream = torch.cuda.Stream()
    for it in items:
        grp.stream.wait_event(it["ready"])
    with torch.cuda.stream(grp.stream):
        outs = run()
        done = torch.cuda.Event()
        done.record()
    return [(o, done) for o in outs]


def _group_sample(self, grp, noisy_latents, eta, generator):
    """`sample_video` inside a launcher lane that carries several examples (`motionclone_amd.launch --batch V`): the host work
    of this example is done; bring it to the lane's group, wait for the fellow members, and take this example's final latents
    from the packed run (None: no fellow is left, the caller runs the one-video loop)."""
    from .. import lanes
    cfg = self.input_config
    ctrl = None
    if self.add_controlnet:      # what single_step_video places at image_index (:176-197)
        ci = self.controlnet_images.to(noisy_latents.device, torch.float16)
        cond, mask = _placed(ci, cfg.image_index, frames=noisy_latents.shape[2])
        ctrl = dict(cond=cond, mask=mask, scale=cfg.controlnet_scale)
    ready = None
    if noisy_latents.is_cuda:
        ready = torch.cuda.Event()
        ready.record()
    item = dict(pipe=self, latents=noisy_latents, text=self.text_embeddings, rep=self.motion_representation_dict, ctrl=ctrl,
                eta=float(eta or 0.0), generator=generator, ready=ready, mask=self._mc_mask[0],
                references=getattr(self, "_mc_refs", None))
    out = grp.meet(lanes.slot_index(), item, lambda items: _run_group(grp, items))
    if out is None:
        return None
    x, done = out
    if done is not None:         # computed in the lane's stream, consumed (decoded) in this thread's
        torch.cuda.current_stream().wait_event(done)
        x.record_stream(torch.cuda.current_stream())
    return x


@torch.no_grad()
def sample_video_batch(self, examples, eta: float = 0.0, decode=True):
    """V examples through ONE packed launch sequence (the way to the packed regime from the pipeline API): what
    `obtain_motion_representation` + `sample_video` do for one example, for a list of V dicts.  Each dict carries one example's
    arguments of those two functions: `new_prompt` (+ `negative_prompt`) or `text_embeddings` [2, n, dim]; `video_latents` or
    `video_path` / `video_data` (+ `duration`); `uncond_embeddings` (optional); `noisy_latents` or `generator`; for
    image-to-video `controlnet_images` or `condition_image_path_list` (either one turns SparseCtrl on; all examples or none);
    `motion_topk` overrides input_config.motion_topk for that example (one value for all the examples of a batch);
    `motion_mask` (tensor or path) is that example's motion mask (default: the pipeline's / the yaml's `motion_mask_path`);
    `motion_references` that example's further motion references (default: the pipeline's / the yaml's `motion_references`).
    Returns a list of V results, each what `sample_video(decode=...)` returns for that example.

    Host work (VAE posterior draw, extraction noise, condition-image VAE draw, CLIP, latent prior) runs per example in list
    order, in the order the two functions run it, from the example's generator: the draws are those of V sequential calls.
    The extraction is one partial forward for the V reference videos, every DDIM step one launch sequence over V times the
    rows (hipGraph replay as in `single_step_video`); `eta > 0` takes the eager steps, the variance noise drawn per video in
    list order at every step.  V = 1 is the two functions themselves."""
    cfg = self.input_config
    V = len(examples)
    if V == 0:
        return []
    use_ctrl = [ex.get("controlnet_images") is not None or ex.get("condition_image_path_list") is not None for ex in examples]
    if any(use_ctrl) != all(use_ctrl):
        raise ValueError("sample_video_batch: " + _MIXED)
    use_ctrl = use_ctrl[0]
    if V == 1:
        ex = examples[0]
        old = {k: getattr(cfg, k) for k in ("new_prompt", "negative_prompt", "video_path", "condition_image_path_list")
               if k in ex and hasattr(cfg, k)}
        try:
            for k in old:
                setattr(cfg, k, ex[k])
            self.obtain_motion_representation(generator=ex.get("generator"), duration=ex.get("duration"), use_controlnet=use_ctrl,
                                              video_latents=ex.get("video_latents"), uncond_embeddings=ex.get("uncond_embeddings"),
                                              video_data=ex.get("video_data"), motion_topk=ex.get("motion_topk"))
            return [self.sample_video(eta=eta, generator=ex.get("generator"), noisy_latents=ex.get("noisy_latents"),
                                      add_controlnet=use_ctrl, text_embeddings=ex.get("text_embeddings"), decode=decode,
                                      controlnet_images=ex.get("controlnet_images"), motion_mask=ex.get("motion_mask"),
                                      motion_references=ex.get("motion_references"))]
        finally:
            for k, v in old.items():
                setattr(cfg, k, v)
    if getattr(cfg, "context_length", None) is not None and _context(cfg, cfg.video_length)[1]:
        raise NotImplementedError("context_length: sample_video_batch with several examples and context windows is not supported")
    topks = [_motion_topk(cfg, ex.get("motion_topk")) for ex in examples]
    if len(set(topks)) != 1:
        raise ValueError("the motion representations of one packed batch differ in their top-k: %s" % topks)
    smp = _sampler(self)
    device = self._execution_device
    step_t = int(cfg.add_noise_step)
    vids, noises, unconds, texts, lats, ext_c, ext_m, smp_c, smp_m = ([] for _ in range(9))
    for ex in examples:                      # host work, example by example in the order of the sequential calls
        gen = ex.get("generator")
        video_latents, video_data = ex.get("video_latents"), ex.get("video_data")
        if video_latents is None:            # obtain_motion_representation (:25-44)
            if video_data is None:
                video_data = video_preprocess(ex.get("video_path", getattr(cfg, "video_path", None)), cfg.height, cfg.width,
                                              cfg.video_length, duration=ex.get("duration"))
            lat = self.vae.encode(video_data.to(self.vae.dtype).to(self.vae.device)).latent_dist.sample(None)
            video_latents = (self.vae.config.scaling_factor * lat).unsqueeze(0).permute(0, 2, 1, 3, 4).contiguous()
        uncond = ex.get("uncond_embeddings")
        if uncond is None:
            tok = self.tokenizer([""], padding="max_length", max_length=self.tokenizer.model_max_length, return_tensors="pt")
            uncond = self.text_encoder(tok.input_ids.to(self.device))[0]
        noises.append(torch.randn(video_latents.shape, generator=gen, device=video_latents.device, dtype=video_latents.dtype))
        vids.append(video_latents)
        unconds.append(uncond.to(video_latents.device))
        if use_ctrl:
            if self.controlnet.use_simplified_condition_embedding:
                src = video_latents
            else:
                if video_data is None:
                    raise ValueError("the pixel-condition SparseCtrl needs the preprocessed frames (video_data)")
                src = ((video_data.unsqueeze(0).to(video_latents.device, video_latents.dtype).permute(0, 2, 1, 3, 4) + 1) / 2)
            c, m = _placed(src, cfg.image_index)
            ext_c.append(c)
            ext_m.append(m)
            ci = _condition_images(self, ex).to(device, torch.float16)           # sample_video (:112-128)
            c, m = _placed(ci, cfg.image_index, frames=cfg.video_length)
            smp_c.append(c)
            smp_m.append(m)
        text = ex.get("text_embeddings")
        if text is None:
            text = self._encode_prompt(ex.get("new_prompt", getattr(cfg, "new_prompt", None)), device, 1, True,
                                       ex.get("negative_prompt", getattr(cfg, "negative_prompt", None)))
        texts.append(text)
        lats.append(self.prepare_latents(1, self.unet.config.in_channels, cfg.video_length, cfg.height, cfg.width, text.dtype,
                                         device, gen, ex.get("noisy_latents")))
    ext_ctrl = None
    ctrls = [None] * V
    if use_ctrl:
        smp.controlnet = self.controlnet.engine()
        ext_ctrl = dict(cond=torch.cat(ext_c, 0).half(), mask=torch.cat(ext_m, 0).half(), scale=cfg.controlnet_scale)
        ctrls = [dict(cond=c, mask=m, scale=cfg.controlnet_scale) for c, m in zip(smp_c, smp_m)]
    reps = smp.extract(torch.cat(vids, 0).half(), torch.cat(noises, 0).half(), torch.cat(unconds, 0).half(),
                       add_noise_step=step_t, ctrl=ext_ctrl, topk=topks[0])
    x = _packed_sample(self, lats, texts, reps, ctrls, eta=eta, generators=[ex.get("generator") for ex in examples],
                       masks=[_motion_mask(self, ex.get("motion_mask"))[0] for ex in examples],
                       references=[_motion_references(self, ex.get("motion_references")) for ex in examples])
    if not decode:
        return [x[v:v + 1].clone() for v in range(V)]     # (a replayed step hands out the graph's static buffer: copies)
    return [self.decode_latents(x[v:v + 1]) for v in range(V)]


@torch.no_grad()
def schedule_customized_step(self, model_output, step_index: int, sample, eta: float = 0.0,
                             use_clipped_model_output: bool = False, generator=None, variance_noise=None,
                             return_dict: bool = True, score=None, guidance_scale=1.0, indices=None,
                             return_middle=False):
    """:285-409, every branch: prediction_type epsilon / sample / v_prediction, clip_sample, use_clipped_model_output,
    eta > 0 (variance noise drawn like randn_tensor or passed in), the score term (optionally on a batch subset
    `indices`), return_middle.  All of it is an affine map of (sample, model_output, score, noise): one elementwise
    kernel (mc_ddim_step_general_f16) in the tensors' own [B, C, F, H, W] layout; the host only derives the scalars."""
    if self.num_inference_steps is None:
        raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
    if model_output.shape[1] == sample.shape[1] * 2 and getattr(self, "variance_type", None) in ["learned", "learned_range"]:
        model_output, _ = torch.split(model_output, sample.shape[1], dim=1)      # :319-322 (IF models)
    cfg = self.config
    t = int(self.timesteps[step_index])
    t_prev = int(self.timesteps[step_index + 1]) if step_index + 1 < len(self.timesteps) else -1
    a_t = float(self.alphas_cumprod[t])
    a_prev = float(self.alphas_cumprod[t_prev]) if t_prev >= 0 else float(self.final_alpha_cumprod)
    sa, sb = a_t ** 0.5, (1.0 - a_t) ** 0.5
    ptype = getattr(cfg, "prediction_type", "epsilon")
    if ptype == "epsilon":
        co = dict(x0_s=1.0 / sa, x0_m=-sb / sa, ep_s=0.0, ep_m=1.0)
    elif ptype == "sample":
        co = dict(x0_s=0.0, x0_m=1.0, ep_s=1.0 / sb, ep_m=-sa / sb)
    elif ptype == "v_prediction":
        co = dict(x0_s=sa, x0_m=-sb, ep_s=sb, ep_m=sa)
    else:
        raise ValueError(f"prediction_type given as {ptype} must be one of `epsilon`, `sample`, or `v_prediction`")
    if getattr(cfg, "thresholding", False):
        raise NotImplementedError("dynamic thresholding (per-sample quantile of |x0|) is not built; the path's scheduler "
                                  "config has thresholding = False")
    clip = float(getattr(cfg, "clip_sample_range", 1.0)) if getattr(cfg, "clip_sample", False) else 0.0
    variance = (1.0 - a_prev) / (1.0 - a_t) * (1.0 - a_t / a_prev)               # _get_variance(timestep, prev_timestep)
    std = float(eta) * max(variance, 0.0) ** 0.5
    guided = score is not None and guidance_scale > 0.0
    co.update(clip=clip, rederive=bool(use_clipped_model_output), sqrt_a=sa, sqrt_b=sb,
              score_coef=float(guidance_scale) * sb if guided else 0.0,
              c_x0=a_prev ** 0.5, c_dir=max(1.0 - a_prev - std * std, 0.0) ** 0.5, c_noise=std)

    if score is not None and return_middle:                                       # :371-372
        _, x0, eps = ops.ddim_step_general(sample, model_output, None, None, co, want_prev=False, want_eps=True)
        return eps.to(model_output.dtype), self.alphas_cumprod[t], \
            (self.alphas_cumprod[t_prev] if t_prev >= 0 else self.final_alpha_cumprod), x0.to(sample.dtype)

    score_full = None
    if guided:
        if indices is not None:
            sel = model_output[indices]
            assert sel.shape == score.shape, "pred_epsilon[indices].shape != score.shape"
            score_full = torch.zeros(model_output.shape, dtype=torch.float32, device=model_output.device)
            score_full[indices] = score.float()                                   # data movement only; arithmetic in the kernel
        else:
            assert model_output.shape == score.shape
            score_full = score.float()
    if eta > 0:
        if variance_noise is not None and generator is not None:
            raise ValueError("Cannot pass both generator and variance_noise. Please make sure that either `generator` or"
                             " `variance_noise` stays `None`.")
        if variance_noise is None:                                               # randn_tensor(shape, generator, device, dtype)
            gdev = generator.device if generator is not None else model_output.device
            variance_noise = torch.randn(model_output.shape, generator=generator, device=gdev,
                                         dtype=model_output.dtype).to(model_output.device)
    else:
        variance_noise = None
    prev, x0, _ = ops.ddim_step_general(sample, model_output, score_full, variance_noise, co, want_x0=return_dict)
    prev = prev.to(sample.dtype)
    if not return_dict:
        return (prev,)
    return prev, x0.to(sample.dtype), (self.alphas_cumprod[t_prev] if t_prev >= 0 else self.final_alpha_cumprod)


def schedule_set_timesteps(self, num_inference_steps: int, guidance_steps: int = 0, guiduance_scale: float = 0.0,
                           device=None, timestep_spacing_type="uneven"):
    """:413-472"""
    ntt = self.config.num_train_timesteps
    if num_inference_steps > ntt:
        raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than `self.config.train_timesteps`:"
                         f" {ntt} as the unet model trained with this scheduler can only handle maximal {ntt} timesteps.")
    self.num_inference_steps = num_inference_steps
    if timestep_spacing_type == "uneven":
        timesteps = uneven_timesteps(num_inference_steps, guidance_steps, guiduance_scale, ntt)
    elif timestep_spacing_type == "linspace":
        timesteps = np.linspace(0, ntt - 1, num_inference_steps).round()[::-1].copy().astype(np.int64)
    elif timestep_spacing_type == "leading":
        ratio = ntt // num_inference_steps
        timesteps = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64) + self.config.steps_offset
    elif timestep_spacing_type == "trailing":
        timesteps = np.round(np.arange(ntt, 0, -ntt / num_inference_steps)).astype(np.int64) - 1
    else:
        raise ValueError(f"{timestep_spacing_type} is not supported. Please make sure to choose one of 'leading' or 'trailing'.")
    self.timesteps = torch.from_numpy(timesteps).to(device)


def unet_customized_forward(self, sample, timestep, encoder_hidden_states, class_labels=None, attention_mask=None,
                            down_block_additional_residuals=None, mid_block_additional_residual=None,
                            return_dict: bool = True, only_motion_feature: bool = False):
    """:478-662 - bound onto the unet by the entry script; delegates to the engine-backed forward."""
    return type(self).forward(self, sample, timestep, encoder_hidden_states, class_labels, attention_mask,
                              down_block_additional_residuals, mid_block_additional_residual, return_dict,
                              only_motion_feature)
