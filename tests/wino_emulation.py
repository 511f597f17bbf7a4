"""Torch (CPU) emulation of csrc/conv_wino_b6.h in the kernel's own operation order: Winograd F(2x2,3x3) of the relevance conv
x * convT(S, W+) with
  * U = G g G^T in fp64 (sums r = 0, 1, 2 then s = 0, 1, 2), rounded once to fp32, split exactly into three bf16 planes;
  * V = B^T d B in fp32, separable, one add or subtract per element and stage, then split exactly;
  * per 16-channel k-step the six plane products, smallest first, each added to an fp32 accumulator that is rounded after every
    product block (one MFMA: the 16 products of bf16 planes are exact, their sum is taken in fp64 here);
  * Y = A^T M A in fp32 in the kernel's order, out = x * Y in fp32."""
import torch

import fp64_anchor as A

G = torch.tensor([[1., 0., 0.], [.5, .5, .5], [.5, -.5, .5], [0., 0., 1.]], dtype=torch.float64)
ORDER = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))     # (plane of V, plane of U): smallest terms first


def wino_u(wp):
    """wp (K, n_oc, 3, 3) = the clamped weights W+ -> U (16, K, n_oc) fp32: the fp64 value of G g G^T, g the flipped kernel"""
    g = wp.flip(2, 3).double()
    t = [sum(G[i, r] * g[:, :, r, :] for r in range(3)) for i in range(4)]                  # (K, n_oc, 3) per i
    u = [[sum(t[i][:, :, s] * G[j, s] for s in range(3)) for j in range(4)] for i in range(4)]
    return torch.stack([u[i][j] for i in range(4) for j in range(4)]).float()


def _bt(d):
    """rows of B^T applied along the first axis of the list d[0..3]"""
    return [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]


def wino_v(s):
    """s (K, hw, hw) fp32 -> V (16, tiles, K) fp32 of the 2x2 output tiles, row-major"""
    K, hw, _ = s.shape
    sp = torch.nn.functional.pad(s, (1, 1, 1, 1))
    th = hw // 2
    d = [[sp[:, a:a + hw - 1:2, b:b + hw - 1:2] for b in range(4)] for a in range(4)]     # d[a][b]: (K, th, th)
    t = [_bt([d[a][b] for a in range(4)]) for b in range(4)]                               # t[b][i]
    v = [_bt([t[b][i] for b in range(4)]) for i in range(4)]                               # v[i][j]
    return torch.stack([v[i][j].reshape(K, th * th).t() for i in range(4) for j in range(4)])


def wino_rel_mul(x, s, wp, pairs=ORDER):
    """x (1, n_oc, hw, hw) >= 0, s (1, K, hw, hw), wp (K, n_oc, 3, 3), all fp32 -> (1, n_oc, hw, hw) fp32 as the kernel computes it"""
    K, n_oc = wp.shape[:2]
    hw = s.shape[-1]
    th = hw // 2
    up = [p.double() for p in A.bf16_split3(wino_u(wp))]        # planes of U: (16, K, n_oc)
    vp = [p.double() for p in A.bf16_split3(wino_v(s[0].float()))]    # planes of V: (16, tiles, K)
    acc = torch.zeros(16, th * th, n_oc)
    for k0 in range(0, K, 16):
        for ia, ib in pairs:
            acc = (acc.double() + torch.bmm(vp[ia][:, :, k0:k0 + 16], up[ib][:, k0:k0 + 16, :])).float()
    m = acc.view(4, 4, th, th, n_oc)
    s0 = [(m[0][j] + m[1][j]) + m[2][j] for j in range(4)]
    s1 = [(m[1][j] - m[2][j]) - m[3][j] for j in range(4)]
    y = torch.empty(hw, hw, n_oc)
    y[0::2, 0::2] = (s0[0] + s0[1]) + s0[2]
    y[0::2, 1::2] = (s0[1] - s0[2]) - s0[3]
    y[1::2, 0::2] = (s1[0] + s1[1]) + s1[2]
    y[1::2, 1::2] = (s1[1] - s1[2]) - s1[3]
    return x * y.permute(2, 0, 1).unsqueeze(0)


def chain_with_wino(layers, weights, saved, r_feat, wino_at):
    """fp64_anchor.vgg_chain in fp32 with the conv layers in `wino_at` evaluated by wino_rel_mul"""
    F = torch.nn.functional
    r = r_feat.float()
    for l in range(len(layers) - 1, -1, -1):
        x = saved[l]
        if layers[l][0] != "conv":
            r = A.maxpool_rule(x, r)
        elif l in wino_at:
            wp = weights[l].clamp(min=0)
            s = A.safe_div(r, F.conv2d(x, wp, padding=1))
            r = wino_rel_mul(x, s, wp)
        else:
            r = A.conv_rule(x, weights[l], r, torch.float32)
    return r
