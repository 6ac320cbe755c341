"""Records what the UNMODIFIED reference code computes for the pin tests, so that they run without the reference tree:

  reference_records.pt        state-dict inventories, tiny UNet forward / extraction / steps (tests/test_oracle_pins.py),
                              checkpoint converters and LoRA merge (tests/test_convert.py)
  reference_controlnet*.pt    SparseControlNet residuals, latent / pixel condition (tests/test_sparsectrl.py)
  reference_ddim_<type>.pt    schedule_customized_step for every branch (tests/test_scheduler_step.py), one file per
                              prediction type

Run where the reference tree exists (oracle/reference_shim.py: MC_REFERENCE_ROOT):  python tests/golden/make_reference_records.py
The inputs are made by the tests' own helpers (seeded); every unseeded input is stored with the outputs."""
import importlib.util
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)
from oracle import reference_shim as shim  # noqa: E402
from oracle import unet3d_ref as U  # noqa: E402
from oracle import vae_ref as V  # noqa: E402


def _pins():
    import test_oracle_pins as T
    inv = {}
    for name, cfg in (("tiny", U.TINY_CONFIG), ("sd15", U.SD15_CONFIG)):
        with torch.device("meta"):
            ref = shim.reference_unet(cfg)
        inv[name] = {k: tuple(v.shape) for k, v in ref.state_dict().items() if "pos_encoder" not in k}
    cfg = U.TINY_CONFIG
    sd = U.random_state_dict(cfg, seed=1234)
    lat, text, vid, noise = T._inputs(cfg)
    N, Gs, gscale = 4, 2, 0.3
    H = shim.RefHarness(cfg, sd, T.HP, N, Gs, gscale)
    out = dict(inventory=inv, timesteps=H.sched.timesteps.clone(), alphas_cumprod=H.sched.alphas_cumprod.clone())
    with torch.no_grad():
        out["eps_b2"] = H.unet(lat.expand(2, -1, -1, -1, -1), int(H.sched.timesteps[0]), encoder_hidden_states=text).sample
    rep = H.extract(vid, noise, text[[0]])
    out["rep"] = {k: [v[0].clone(), v[1].clone()] for k, v in rep.items()}
    out["rep_keys"] = list(rep)
    nxt = H.step(lat, 0, text, rep)
    p = H.step(nxt, Gs, text, rep)
    last = H.step(p, N - 1, text, rep)
    out.update(guided_next=nxt.clone(), plain_next=p.clone(), last_next=last.clone())
    return out


def _controlnet(pixel):
    import test_sparsectrl as T
    from motionclone.models.sparse_controlnet import SparseControlNetModel
    cfg = dict(U.TINY_CONFIG)
    ref = SparseControlNetModel(
        in_channels=4, down_block_types=("CrossAttnDownBlock3D",) * 3 + ("DownBlock3D",),
        block_out_channels=cfg["block_out_channels"], layers_per_block=2, cross_attention_dim=cfg["cross_attention_dim"],
        attention_head_dim=cfg["attention_heads"], num_attention_heads=cfg["attention_heads"],
        set_noisy_sample_input_to_zero=True, use_simplified_condition_embedding=not pixel, conditioning_channels=3 if pixel else 4,
        motion_module_kwargs=dict(num_attention_heads=cfg["motion_heads"], num_transformer_block=1,
                                  attention_block_types=["Temporal_Self"], temporal_position_encoding=True,
                                  temporal_position_encoding_max_len=32, temporal_attention_dim_div=1)).float()
    ref.controlnet_cond_embedding.float()
    shapes = {k: tuple(v.shape) for k, v in ref.state_dict().items() if "pos_encoder" not in k}
    sd = (U.random_controlnet_state_dict(cfg, conditioning_channels=3, simplified=False) if pixel
          else U.random_controlnet_state_dict(cfg))
    ref.load_state_dict(sd, strict=False)
    text = torch.randn(2, 7, cfg["cross_attention_dim"], generator=torch.Generator().manual_seed(7))
    cond, mask = T.pixel_cond_inputs() if pixel else T.cond_inputs()
    lat = torch.randn(2, 4, 2 if pixel else 4, 8, 8, generator=torch.Generator().manual_seed(23))
    real_to = torch.Tensor.to

    def keep_fp32(self, *a, **k):   # the reference hard-casts the condition to fp16 (sparse_controlnet.py:523)
        return self if (a and a[0] is torch.float16) else real_to(self, *a, **k)
    torch.Tensor.to = keep_fp32
    try:
        with torch.no_grad():
            d_ref, m_ref = ref(lat, 500, encoder_hidden_states=text, controlnet_cond=cond, conditioning_mask=mask,
                               conditioning_scale=0.7, guess_mode=False, return_dict=False)
    finally:
        torch.Tensor.to = real_to
    return dict(shapes=shapes, lat=lat, down=[t.clone() for t in d_ref], mid=m_ref.clone())


def _ref_module(name):
    path = os.path.join(shim.REFERENCE_ROOT, "motionclone", "utils", name + ".py")
    spec = importlib.util.spec_from_file_location("_ref_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _as_sources(out, inp):
    """a converter's output as {key: (input key, shape)} where the tensor is a view of one input tensor with the same
    values, else {key: tensor}"""
    by_ptr = {}
    for k, v in inp.items():
        by_ptr.setdefault(v.untyped_storage().data_ptr(), []).append(k)
    rec = {}
    for k, v in out.items():
        src = [s for s in by_ptr.get(v.untyped_storage().data_ptr(), [])
               if inp[s].numel() == v.numel() and torch.equal(inp[s].reshape(v.shape), v)]
        rec[k] = (src[0], tuple(v.shape)) if src else v.clone()
    return rec


def _convert():
    import test_convert as T
    R = _ref_module("convert_from_ckpt")
    sd = U.random_state_dict(U.TINY_CONFIG, seed=3)
    unet_sd = {k: v for k, v in sd.items() if "motion_modules" not in k}
    ldm = T.unet_to_ldm(unet_sd)
    cfg = dict(layers_per_block=2, class_embed_type=None)
    unet = _as_sources(R.convert_ldm_unet_checkpoint(dict(ldm), cfg), ldm)
    vsd = {k: torch.randn(s) if len(s) < 3 else torch.zeros(s) for k, s in V.param_shapes(V.SD15_VAE_CONFIG).items()}
    vldm = T.vae_to_ldm(vsd, 4)
    ref_cfg = dict(down_block_types=["DownEncoderBlock2D"] * 4, up_block_types=["UpDecoderBlock2D"] * 4)
    vae = _as_sources(R.convert_ldm_vae_checkpoint(dict(vldm), ref_cfg), vldm)
    clip = {"cond_stage_model.transformer.text_model.embeddings.token_embedding.weight": torch.ones(3, 2),
            "model.diffusion_model.out.2.bias": torch.zeros(4)}
    clip_out = {k: v.clone() for k, v in R.convert_ldm_clip_checkpoint_concise(clip).items()}
    # LoRA merge: the reference's weights after convert_lora(alpha 0.8) + load_diffusers_lora(alpha 1.0) on the toy UNet
    RL = _ref_module("convert_lora_safetensor_to_diffusers")
    import types
    kohya, diff = T._lora_sd(1)
    torch.manual_seed(0)
    b = T._toy_unet()
    w0 = {k: v.detach().clone() for k, v in b.state_dict().items()}
    pb = types.SimpleNamespace(unet=b, text_encoder=None)
    RL.convert_lora(pb, kohya, alpha=0.8)
    RL.load_diffusers_lora(pb, diff, alpha=1.0)
    lora = dict(before=w0, after={k: v.detach().clone() for k, v in b.state_dict().items()})
    return dict(unet=unet, vae=vae, vae_ldm_zero_keys=sorted(k for k, v in vldm.items() if not v.any()), clip=clip_out, lora=lora)


def _ddim():
    import test_scheduler_step as T
    import motionclone.utils.motionclone_functions as ref      # the reference's module (shim.install put it first on sys.path)
    assert ref.__file__.startswith(shim.REFERENCE_ROOT)
    sample, mo, score, noise = T._tensors()
    recs = {}
    for case in T.CASES:
        sch = shim.DDIMScheduler(beta_start=0.00085, beta_end=0.012, steps_offset=1, clip_sample=case["clip_sample"],
                                 prediction_type=case["prediction_type"])
        sch.variance_type = "fixed_small"
        sch.customized_step = ref.schedule_customized_step.__get__(sch)
        sch.customized_set_timesteps = ref.schedule_set_timesteps.__get__(sch)
        sch.customized_set_timesteps(6, 3, 0.4, device="cpu", timestep_spacing_type="uneven")
        steps = {}
        for step_index in (0, 5):
            kw = dict(eta=case["eta"], use_clipped_model_output=case["use_clipped_model_output"],
                      variance_noise=noise if case["eta"] > 0 else None)
            full = sch.customized_step(mo.clone(), step_index, sample, score=score, guidance_scale=0.6, **kw)
            subset = sch.customized_step(mo.clone(), step_index, sample, score=score[1:2], guidance_scale=0.6, indices=[1], **kw)
            middle = sch.customized_step(mo.clone(), step_index, sample, score=score, return_middle=True, **kw)
            steps[step_index] = dict(full=(full[0].clone(), full[1].clone(), float(full[2])), subset=subset[0].clone(),
                                     middle=(middle[0].clone(), middle[3].clone()))
        recs[T.case_id(case)] = dict(timesteps=sch.timesteps.clone(), alphas_cumprod=sch.alphas_cumprod.clone(),
                                     final_alpha_cumprod=sch.final_alpha_cumprod.clone(), steps=steps)
    return recs


def main():
    shim.install()
    for name, rec in (("reference_records.pt", dict(pins=_pins(), convert=_convert())),
                      ("reference_controlnet.pt", _controlnet(False)), ("reference_controlnet_pixel.pt", _controlnet(True))):
        path = os.path.join(HERE, name)
        torch.save(rec, path)
        print("wrote", path, os.path.getsize(path), "bytes")
    ddim = _ddim()
    for ptype in ("epsilon", "sample", "v_prediction"):
        path = os.path.join(HERE, "reference_ddim_%s.pt" % ptype)
        torch.save({k: v for k, v in ddim.items() if k.startswith(ptype + "-")}, path)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
