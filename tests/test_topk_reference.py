"""The engine's top-k loss / seed kernels against what the UNMODIFIED reference consumer computes for a k = 3 representation
(tests/golden/reference_topk.pt, recorded by tests/golden/make_topk_records.py through oracle/reference_shim: the reference's
get_temp_attn_prob -> compute_temp_loss -> torch.autograd.grad on the recorded q / k of two hooked temporal attentions of the
tiny UNet).  This is the proof that the reference's consumer is k-general and that the kernels agree with it.  Bounds are
those of tests/test_kernels.py::test_temporal_attention_and_guidance for the same quantities.  CPU (host simulator) only;
the test does not read the reference tree."""
import os

import torch

from motionclone_amd import ops

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_topk.pt")


def close(a, b, atol, rtol, what=""):
    err = (a.float() - b.float()).abs()
    tol = atol + rtol * b.float().abs()
    assert torch.isfinite(a.float()).all(), what + ": non-finite output"
    assert (err <= tol).all(), "%s: max err %.4g (ref max %.3g)" % (what, err.max().item(), b.abs().max().item())


def _tokens(x):   # the reference's [(b p), F, C] (b = 1) -> the engine's token rows [(f p), C]
    return x.permute(1, 0, 2).reshape(-1, x.shape[2]).contiguous()


def test_topk_loss_and_seed_match_the_reference_consumer(emu_device):
    rec = torch.load(RECORD)
    K, weight, heads = rec["K"], rec["weight"], rec["heads"]
    assert K == 3 and len(rec["modules"]) == 2
    total = 0.0
    for name, m in rec["modules"].items():
        HW, F_, C = m["q"].shape
        d = C // heads
        assert m["idx"].shape == m["val"].shape == (HW, heads, F_, K) and m["idx"].dtype == torch.uint8
        qk = torch.cat([_tokens(m["q"]), _tokens(m["k"]), torch.zeros(F_ * HW, C, dtype=torch.float16)], 1)
        q, k, v = qk[:, :C], qk[:, C:2 * C], qk[:, 2 * C:]
        idx, val = m["idx"].contiguous(), m["val"].float().contiguous()
        # the reference's own gather on the engine's probabilities: the representation's layout means the same on both sides
        P = ops.tattn_prob(q, k, 1, F_, HW, heads, d).float()
        lm = ops.tattn_loss(q, k, idx, val, 1, F_, HW, heads, d)
        assert abs(lm.item() - torch.nn.functional.mse_loss(torch.gather(P, -1, idx.long()), val).item()) < 2e-3
        total += lm.item()
        g = torch.ones_like(qk)
        ops.tattn_bwd(q, k, v, None, g[:, :C], g[:, C:2 * C], g[:, 2 * C:], 1, F_, HW, heads, d, ref_idx=idx, ref_val=val,
                      seed_coef=weight * 2.0 / idx.numel())
        print(name, "loss", lm.item(), "|dq| max", m["dq"].abs().max().item(), "|dk| max", m["dk"].abs().max().item())
        assert m["dq"].abs().max() > 0.05 and m["dk"].abs().max() > 0.05     # the bounds below bite
        close(g[:, :C], _tokens(m["dq"]), 2e-3, 2e-2, name + " dq")
        close(g[:, C:2 * C], _tokens(m["dk"]), 2e-3, 2e-2, name + " dk")
        assert g[:, 2 * C:].abs().max() == 0
    ref = float(rec["loss"])
    print("loss", total, "reference", ref)
    assert abs(total - ref) < 2e-3 * max(1.0, abs(ref)) + 1e-5
