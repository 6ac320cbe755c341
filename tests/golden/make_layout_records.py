"""Records what the UNMODIFIED reference UNet3DConditionModel computes for the AnimateDiff v1 / v2 model layouts, so that
tests/test_layouts_engine.py and tests/test_layouts_api.py run without the reference tree:

  reference_layouts.pt   per layout (tests/layout_util.py: a = video-wide GroupNorm, b = mid-block motion module hooked through
                         ["mid_block", "up_blocks.1"], c = both + decoder-only): eps of one B = 2 forward, the representation of
                         an extraction, loss and latent gradient of one guided step (compute_temp_loss + torch.autograd.grad as
                         they are), the latents after one guided and one plain step; the state-dict key list of every layout
                         and of the structural one (motion_module_resolutions = [1, 2]); the sensitivity figures below.

Results only: weights come from seeds (oracle.unet3d_ref.random_state_dict + layout_util.mid_motion_tensors).

Sensitivity: with N(0, 0.02) the mid-block module's proj_out moves eps by less than the 2e-2 parity bound, so its proj_out is
scaled (a power of two, recorded) until the reference's eps with and without the module differ by >= 0.1 relative L2; the same
is asserted for video-wide against per-frame GroupNorm.  Both figures go into the file's metadata.

Run where the reference tree exists (oracle/reference_shim.py: MC_REFERENCE_ROOT):  python tests/golden/make_layout_records.py"""
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)
from oracle import reference_shim as shim  # noqa: E402
from oracle import unet3d_ref as U  # noqa: E402
import layout_util as LU  # noqa: E402

MIN_VISIBLE = 0.1      # 5 x the 2e-2 parity bound of eps


def reference_unet(switches):
    shim.install()
    from motionclone.models.unet import UNet3DConditionModel
    cfg = U.TINY_CONFIG
    kw = dict(shim.SD15_UNET_CONFIG)
    kw.update(block_out_channels=tuple(cfg["block_out_channels"]), cross_attention_dim=cfg["cross_attention_dim"],
              attention_head_dim=cfg["attention_heads"], layers_per_block=cfg["layers_per_block"])
    mk = dict(shim.MOTION_KWARGS)
    mk["motion_module_kwargs"] = dict(shim.MOTION_KWARGS["motion_module_kwargs"], num_attention_heads=cfg["motion_heads"])
    kw.update(mk)
    kw.update(unet_use_cross_frame_attention=False, unet_use_temporal_attention=False)
    kw.update(switches)
    return UNet3DConditionModel(**kw)


class Harness:
    """the reference's guidance functions bound the way oracle.reference_shim.RefHarness binds them (t2v_video_sample.py
    :57-72), on a reference UNet of the given layout"""

    def __init__(self, switches, sd, hooks):
        import motionclone.utils.motionclone_functions as mf
        unet = reference_unet(switches)
        missing, unexpected = unet.load_state_dict(sd, strict=False)
        assert not unexpected, unexpected
        assert all("pos_encoder" in m for m in missing), missing
        unet.eval()
        for p in unet.parameters():
            p.requires_grad = False
        hp = LU.HP
        cfgns = types.SimpleNamespace(motion_guidance_blocks=list(hooks), guidance_steps=LU.G_STEPS,
                                      warm_up_steps=hp["warm_up_steps"], cool_up_steps=hp["cool_up_steps"],
                                      cfg_scale=hp["cfg_scale"], motion_guidance_weight=hp["motion_guidance_weight"])
        sched = shim.DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
        sched.customized_step = mf.schedule_customized_step.__get__(sched)
        sched.customized_set_timesteps = mf.schedule_set_timesteps.__get__(sched)
        unet.forward = mf.unet_customized_forward.__get__(unet)
        pipe = types.SimpleNamespace(unet=unet, scheduler=sched, input_config=cfgns, add_controlnet=False)
        unet.input_config = cfgns
        for fn in ("single_step_video", "get_temp_attn_prob", "compute_temp_loss", "add_noise"):
            setattr(pipe, fn, getattr(mf, fn).__get__(pipe))
        mf.prep_unet_attention(unet, cfgns.motion_guidance_blocks)
        mf.prep_unet_conv(unet)
        sched.customized_set_timesteps(LU.N_STEPS, LU.G_STEPS, LU.G_SCALE, device="cpu", timestep_spacing_type="uneven")
        self.pipe, self.unet, self.sched = pipe, unet, sched

    def eps2(self, lat, t, text):
        with torch.no_grad():
            return self.unet(lat.expand(2, -1, -1, -1, -1), t, encoder_hidden_states=text).sample.clone()

    def extract(self, vid, noise, uncond_text):
        with torch.no_grad():
            noisy = self.pipe.add_noise(400, vid, noise)
            self.unet(noisy, 400, encoder_hidden_states=uncond_text, return_dict=False, only_motion_feature=True)
            prob = self.pipe.get_temp_attn_prob()
            # (the gap between the two best probabilities of every row: an arg-max may differ from the recorded one at a tie only)
            self.gap = {k: (lambda v: (v[..., 0:1] - v[..., 1:2]).half())(torch.topk(t, k=2, dim=-1)[0]) for k, t in prob.items()}
            return {k: [v.clone(), i.to(torch.uint8)] for k, t in prob.items() for v, i in [torch.topk(t, k=1, dim=-1)]}

    def loss_and_grad(self, lat, step_index, text, rep):
        """the guided branch of single_step_video up to the gradient (:210-236), as it is"""
        pipe, hp = self.pipe, LU.HP
        pipe.motion_representation_dict = rep
        t = self.sched.timesteps[step_index]
        control = lat.clone().detach()
        control.requires_grad = True
        self.unet(control, t, encoder_hidden_states=text[[1]])
        loss = hp["motion_guidance_weight"] * pipe.compute_temp_loss(pipe.get_temp_attn_prob())
        if step_index < hp["warm_up_steps"]:
            loss = (step_index + 1) / hp["warm_up_steps"] * loss
        if step_index > LU.G_STEPS - hp["cool_up_steps"]:
            loss = (LU.G_STEPS - step_index) / hp["cool_up_steps"] * loss
        grad = torch.autograd.grad(loss, control, allow_unused=True)[0]
        return loss.detach().clone(), grad.detach().clone()

    def step(self, lat, step_index, text, rep):
        pipe = self.pipe
        pipe.text_embeddings = text
        pipe.motion_representation_dict = rep
        pipe.motion_scale = pipe.input_config.motion_guidance_weight
        return pipe.single_step_video(lat, step_index, self.sched.timesteps[step_index], {}).clone()


def main():
    shim.install()
    lat, text, vid, noise = LU.inputs()
    t0 = 701
    meta = {}
    # ---- sensitivity: the mid-block module must move eps by >= MIN_VISIBLE, video-wide GroupNorm likewise ----------------
    sw_b, keys_b, hooks_b = LU.LAYOUTS["b"]
    base = Harness({}, LU.layout_state_dict({}), ["up_blocks.1"]).eps2(lat, t0, text)
    scale, moved = 1.0, 0.0
    while True:
        moved = LU.rel(Harness(sw_b, LU.layout_state_dict(keys_b, scale), hooks_b).eps2(lat, t0, text), base)
        if moved >= MIN_VISIBLE:
            break
        scale *= 2.0
        assert scale <= 4096.0, (scale, moved)
    sw_a, keys_a, hooks_a = LU.LAYOUTS["a"]
    wide = LU.rel(Harness(sw_a, LU.layout_state_dict(keys_a), hooks_a).eps2(lat, t0, text), base)
    assert moved >= MIN_VISIBLE and wide >= MIN_VISIBLE, (moved, wide)
    meta.update(mid_proj_out_scale=scale, eps_moved_by_mid_module=moved, eps_moved_by_video_wide_groupnorm=wide,
                t_forward=t0, frames=LU.F, grid=(LU.H, LU.W))
    print("sensitivity:", meta)
    out = dict(meta=meta, layouts={}, keys={})
    for name, (sw, keys, hooks) in LU.LAYOUTS.items():
        sd = LU.layout_state_dict(keys, scale)
        Hn = Harness(sw, sd, hooks)
        rep = Hn.extract(vid, noise, text[[0]])
        loss, grad = Hn.loss_and_grad(lat, 0, text, rep)
        guided = Hn.step(lat, 0, text, rep)
        plain = Hn.step(guided, LU.G_STEPS, text, rep)
        hooked = [n for n, m in Hn.unet.named_modules() if type(m).__name__ == "VersatileAttention"
                  and any(b in n for b in hooks)]
        assert list(rep) == hooked
        out["layouts"][name] = dict(eps=Hn.eps2(lat, t0, text).half(), rep={k: [v[0].half(), v[1]] for k, v in rep.items()}, gap=Hn.gap,
                                    loss=loss, grad=grad, guided=guided.half(), plain=plain.half(), hooked=hooked)
        out["keys"][name] = LU.pack_keys([k for k in Hn.unet.state_dict() if "pos_encoder" not in k])
        if name == "b":     # where the reference's named_modules() puts the mid-block attentions among all temporal attentions
            names = [n for n, m in Hn.unet.named_modules() if type(m).__name__ == "VersatileAttention"]
            meta["first_mid_attention_index"] = (names.index(LU.MID + "temporal_transformer.transformer_blocks.0.attention_blocks.0"),
                                                 len(names))
        print(name, "loss", float(loss), "|grad|", float(grad.norm()), "hooked", len(hooked))
    sw, keys, hooks = LU.RES12
    un = reference_unet(sw)
    out["keys"]["res12"] = LU.pack_keys([k for k in un.state_dict() if "pos_encoder" not in k])
    out["layouts"]["res12"] = dict(hooked=[n for n, m in un.named_modules() if type(m).__name__ == "VersatileAttention"
                                           and any(b in n for b in hooks)])
    path = os.path.join(HERE, "reference_layouts.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes", meta)


if __name__ == "__main__":
    main()
