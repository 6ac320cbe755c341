"""Records what the UNMODIFIED reference consumer computes for a top-k (k = 3) motion representation, so that
tests/test_topk_reference.py runs without the reference tree:

  reference_topk.pt    for two hooked temporal attentions of the tiny UNet: the recorded q / k, a k = 3 representation of
                       ANOTHER video, compute_temp_loss over the two modules and the gradient of weight x loss w.r.t. q / k

The reference's producer is torch.topk(k = 1) (motionclone_functions.py:79); its consumer compute_temp_loss (:85-100) gathers
with whatever index tensor the representation holds.  Here the representation is torch.topk(k = 3) of the reference's own
get_temp_attn_prob, and get_temp_attn_prob -> compute_temp_loss -> torch.autograd.grad run as they are.

Run where the reference tree exists (oracle/reference_shim.py: MC_REFERENCE_ROOT):  python tests/golden/make_topk_records.py"""
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

K = 3
WEIGHT = 3000.0
HOOKED = ["up_blocks.1.motion_modules.2"]     # its two temporal attentions
HP = dict(cfg_scale=7.5, motion_guidance_weight=2000.0, warm_up_steps=10, cool_up_steps=10)


def main():
    shim.install()
    cfg = U.TINY_CONFIG
    sd = U.random_state_dict(cfg, seed=1234)
    H = shim.RefHarness(cfg, sd, HP, 4, 2, 0.3)
    pipe = H.pipe
    # the read-out and the loss see the two attentions of HOOKED only (the UNet keeps its own config: up_blocks.1)
    pipe.input_config = types.SimpleNamespace(**dict(vars(pipe.input_config), motion_guidance_blocks=HOOKED))
    g = torch.Generator().manual_seed(31)
    F_, Hh, Ww = 6, 8, 8
    vid = 0.18215 * torch.randn(1, 4, F_, Hh, Ww, generator=g)
    noise = torch.randn(1, 4, F_, Hh, Ww, generator=g)
    lat = torch.randn(1, 4, F_, Hh, Ww, generator=g)
    text = torch.randn(2, 7, cfg["cross_attention_dim"], generator=g)
    with torch.no_grad():
        noisy = pipe.add_noise(400, vid, noise)
        H.unet(noisy, 400, encoder_hidden_states=text[[0]], return_dict=False, only_motion_feature=True)
        rep = {k: [v.clone(), i.to(torch.uint8)] for k, t in pipe.get_temp_attn_prob().items()
               for v, i in [torch.topk(t, k=K, dim=-1)]}
        H.unet(lat, int(H.sched.timesteps[0]), encoder_hidden_states=text[[1]], return_dict=False, only_motion_feature=True)
    assert len(rep) == 2, list(rep)
    mods = dict(H.unet.named_modules())
    leaves = {}
    for name in rep:     # the recorded q / k, rounded to fp16 (what the engine stores), as the leaves of the loss
        proc = mods[name].processor
        proc.query = proc.query.detach().half().float().requires_grad_()
        proc.key = proc.key.detach().half().float().requires_grad_()
        leaves[name] = (proc.query, proc.key)
    pipe.motion_representation_dict = rep
    loss = pipe.compute_temp_loss(pipe.get_temp_attn_prob())
    flat = [t for name in rep for t in leaves[name]]
    grads = torch.autograd.grad(WEIGHT * loss, flat)
    out = dict(K=K, weight=WEIGHT, heads=cfg["motion_heads"], loss=loss.detach().clone(), modules={})
    for n, name in enumerate(rep):
        q, k = leaves[name]
        out["modules"][name] = dict(q=q.detach().half(), k=k.detach().half(), val=rep[name][0].clone(), idx=rep[name][1].clone(),
                                    dq=grads[2 * n].clone(), dk=grads[2 * n + 1].clone())
    path = os.path.join(HERE, "reference_topk.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes; loss", float(loss),
          {k: tuple(v["q"].shape) for k, v in out["modules"].items()})


if __name__ == "__main__":
    main()
