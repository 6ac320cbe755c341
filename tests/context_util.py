"""fp64 restatement of the context-window blend (shared by the context tests): the per-frame weighted average of the windows'
whole updates, written from the rule's definition - independent of the kernel's index arithmetic."""
import torch


def tokens_to_latent(tok, nW, CL, L, H, W):
    """token rows [(w j y x), >= CL] -> [nW, CL, L, H, W] float64"""
    return tok[:, :CL].double().reshape(nW, L, H, W, CL).permute(0, 4, 1, 2, 3).contiguous()


def weights64(L, kind):
    return [1.0] * L if kind == "uniform" else [float(min(j + 1, L - j)) for j in range(L)]


def cover(f, starts, L):
    return [w for w, s in enumerate(starts) if s <= f < s + L]


def blend_update_f64(ec, eu, x, score, starts, L, wt, cfg, a_t, a_prev, coef, sigma=0.0):
    """ec / eu / score: [nW, CL, L, H, W] (score may be None), x [1, CL, F, H, W]; returns (out, eps) float64 [1, CL, F, H, W]"""
    x = x.double()
    F = x.shape[2]
    out, eps_all = torch.zeros_like(x), torch.zeros_like(x)
    c_dir = max(1.0 - a_prev - sigma ** 2, 0.0) ** 0.5
    for f in range(F):
        ws = cover(f, starts, L)
        assert ws, "frame %d is not covered" % f
        Z = sum(wt[f - starts[w]] for w in ws)
        eps = torch.zeros_like(x[0, :, f])
        sc = torch.zeros_like(eps)
        for w in ws:
            j = f - starts[w]
            a = wt[j] / Z
            c, u = ec[w, :, j].double(), eu[w, :, j].double()
            eps = eps + a * (c + cfg * (c - u))
            if score is not None:
                sc = sc + a * score[w, :, j].double()
        x0 = (x[0, :, f] - (1.0 - a_t) ** 0.5 * eps) / a_t ** 0.5
        out[0, :, f] = a_prev ** 0.5 * x0 + c_dir * (eps - coef * sc)
        eps_all[0, :, f] = eps
    return out, eps_all
