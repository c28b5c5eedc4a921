"""CPU restatement of the reference's DiscriminatorP / MultiPeriodDiscriminator forward (hifigan_infer/hifigan_model.py:127-187)
in torch CPU ops (F.pad reflect, F.conv2d, F.leaky_relu), parametrised by dtype: fp64 autograd over it is the yardstick of
tests/test_gpu_hifigan_mpd.py, fp32 autograd over it gives the "fp32 CPU deviation" its bounds are made of.  Also the seeded makers
of state dicts, audio and upstream gradients, the row arithmetic of the plan, and the edge lengths per period."""
import torch
import torch.nn.functional as F

PERIODS = (2, 3, 5, 7, 11)
WIDTHS = (1, 32, 128, 512, 1024, 1024, 1)
SLOPE = 0.1
N_LAYERS = 6


def layer_names(d):
    return [f"discriminators.{d}.convs.{m}" for m in range(5)] + [f"discriminators.{d}.conv_post"]


def make_state_dict(seed, periods=PERIODS):
    """Reference-keyed, Conv2d-shaped, weight-normed: bias, weight_g [Cout,1,1,1], weight_v [Cout,Cin,k,1] per conv.  weight_g is not
    ||weight_v||, so the norm's own gradient is exercised; the scale keeps the feature maps of order 1 through six layers."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for d in range(len(periods)):
        for i, name in enumerate(layer_names(d)):
            cin, cout, k = WIDTHS[i], WIDTHS[i + 1], 5 if i < 5 else 3
            v = torch.randn(cout, cin, k, 1, generator=g) * (2.0 / (cin * k)) ** 0.5
            sd[name + ".bias"] = (torch.rand(cout, generator=g) - 0.5) * 0.2
            sd[name + ".weight_g"] = v.flatten(1).norm(dim=1).view(-1, 1, 1, 1) * (0.8 + 0.4 * torch.rand(cout, 1, 1, 1, generator=g))
            sd[name + ".weight_v"] = v
    return sd


def make_audio(B, T, seed):
    return torch.tanh(torch.randn(B, 1, T, generator=torch.Generator().manual_seed(seed))) * 0.5


def rows(period, T):
    """[H0, H1, .., H6]: rows of the padded audio viewed [H0, period] and of the six feature maps; raises where torch's reflect pad does."""
    pad = (period - T % period) % period
    if pad > T - 1:
        raise ValueError(f"T={T} too short for the reflect padding of {pad} at period {period}")
    H = [(T + pad) // period]
    for i in range(4):
        H.append((H[-1] - 1) // 3 + 1)
    return H + [H[-1], H[-1]]


def disc_forward(params, period, x, dtype):
    """params: the six (weight_v, weight_g, bias) of one DiscriminatorP, any dtype; x [B, 1, T].  -> (score [B, H*p], the six feature maps)."""
    x = x.to(dtype)
    b, c, t = x.shape
    if t % period != 0:
        x = F.pad(x, (0, period - t % period), "reflect")
    x = x.view(b, c, -1, period)
    fmap = []
    for i, (v, g, bias) in enumerate(params):
        v, g, bias = v.to(dtype), g.to(dtype), bias.to(dtype)
        w = v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1, 1))
        if i < 5:
            x = F.leaky_relu(F.conv2d(x, w, bias, stride=(3 if i < 4 else 1, 1), padding=(2, 0)), SLOPE)
        else:
            x = F.conv2d(x, w, bias, stride=1, padding=(1, 0))
        fmap.append(x)
    return torch.flatten(x, 1, -1), fmap


def disc_params(sd, d):
    return [(sd[n + ".weight_v"], sd[n + ".weight_g"], sd[n + ".bias"]) for n in layer_names(d)]


def mpd_forward(sd, y, y_hat, dtype, periods=PERIODS):
    outs = ([], [], [], [])
    for d, p in enumerate(periods):
        params = disc_params(sd, d)
        s_r, f_r = disc_forward(params, p, y, dtype)
        s_g, f_g = disc_forward(params, p, y_hat, dtype)
        for o, v in zip(outs, (s_r, s_g, f_r, f_g)):
            o.append(v)
    return outs


def make_upstream(period, B, T, seed):
    """A seeded random weight for every feature map of one discriminator over B items, and for the score: seven tensors."""
    g = torch.Generator().manual_seed(seed)
    H = rows(period, T)
    ups = [torch.randn(B, WIDTHS[i + 1], H[i + 1], period, generator=g) for i in range(N_LAYERS)]
    return ups + [torch.randn(B, H[6] * period, generator=g)]


def weighted_sum(score, fmap, ups):
    """sum_l sum(fmap_l * g_l) + sum(score * g_score): injects a gradient at every layer."""
    total = (score * ups[N_LAYERS].to(score.dtype)).sum()
    for f, u in zip(fmap, ups):
        total = total + (f * u.to(f.dtype)).sum()
    return total


def disc_grads(sd, d, period, x, ups, dtype):
    """Gradients of weighted_sum for discriminator d on x [B, 1, T]: ({key: grad} over its 18 parameters and "x", score, fmaps)."""
    names = layer_names(d)
    leaves = {n + s: sd[n + s].to(dtype).clone().requires_grad_(True) for n in names for s in (".bias", ".weight_g", ".weight_v")}
    xl = x.to(dtype).clone().requires_grad_(True)
    params = [(leaves[n + ".weight_v"], leaves[n + ".weight_g"], leaves[n + ".bias"]) for n in names]
    score, fmap = disc_forward(params, period, xl, dtype)
    weighted_sum(score, fmap, ups).backward()
    out = {k: v.grad.detach() for k, v in leaves.items()}
    out["x"] = xl.grad.detach()
    return out, score.detach(), [f.detach() for f in fmap]


def length_for(period, layer, n_rows, rem=0):
    """The smallest T with T % period == rem whose feature map `layer` has n_rows rows."""
    T = max(period, 1)
    while True:
        if T % period == rem:
            try:
                if rows(period, T)[layer + 1] == n_rows:
                    return T
            except ValueError:
                pass
        T += 1


def edge_lengths(period):
    """{what it probes: (B, T)} per period; the plan test pins the rows and tiles these give.
    reflect:  T % p == 0 with H = 1 (T = p), pad p - 1 at the shortest legal T of that kind (T = p + 1), pad 1 (T = 2p - 1)
    phases:   H0 % 3 = 2, 0, 1 at the first strided conv (H0 = 8, 9, 10), and H1 % 3 = 0, 1, 2 at the second (H0 = 9, 10, 13)
    tiles:    conv 1 (32 -> 128) with N = H2 * p at the 128-column tile's edge.  127 is prime and 128 = 2^7, 129 = 3 * 43, so
              N = 128 exists at p = 2 only, 129 at p = 3 only and 127 at none: every period takes the largest multiple of p
              that is <= 127 and the smallest that is >= 129, and p = 2, 3 also 128, 129 themselves
    several:  T = 2051 (pad where 2051 % p != 0): conv 0 and conv 1 span several tiles
    tails:    T = 1000: two rows at the 1024-wide layers for p = 7 and 11; T = p + 1 and 2p - 1 give one row"""
    p = period
    out = {"H1": (1, p), "pad_p-1": (3, p + 1), "pad_1": (1, 2 * p - 1), "phase_H0=8": (3, 8 * p), "phase_H0=9": (1, 9 * p),
           "phase_H0=10": (3, 10 * p - 1), "phase_H0=13": (1, 13 * p), "several_tiles": (1, 2051), "tails": (1, 1000)}
    lo, hi = 127 // p, -(-129 // p)
    out[f"tile_N={lo * p}"] = (3, length_for(p, 1, lo, rem=0))
    out[f"tile_N={hi * p}"] = (1, length_for(p, 1, hi, rem=1 if p > 2 else 0))
    if 128 % p == 0:
        out["tile_N=128"] = (3, length_for(p, 1, 128 // p, rem=1))
    if 129 % p == 0:
        out["tile_N=129"] = (3, length_for(p, 1, 129 // p, rem=p - 1))
    return out


def disc_loss(sd, y, y_hat, dtype, periods=PERIODS):
    """The reference's discriminator_loss (hifigan_model.py:259-270) over mpd_forward: sum_d mean((1 - d(y))^2) + mean(d(y_hat)^2)."""
    s_r, s_g, _, _ = mpd_forward(sd, y, y_hat, dtype, periods)
    return sum(((1 - r) ** 2).mean() + (g ** 2).mean() for r, g in zip(s_r, s_g))


def sgd_steps(sd, y, y_hat, dtype, lr, n):
    """p -= lr * grad of disc_loss, n times: (the loss before every step and after the last, the parameters at the end)."""
    ps = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    losses = []
    for _ in range(n):
        loss = disc_loss(ps, y, y_hat, dtype)
        grads = torch.autograd.grad(loss, list(ps.values()))
        losses.append(float(loss.detach()))
        with torch.no_grad():
            for p, g in zip(ps.values(), grads):
                p -= lr * g
    with torch.no_grad():
        losses.append(float(disc_loss(ps, y, y_hat, dtype)))
    return losses, {k: v.detach() for k, v in ps.items()}


MARGIN = 2e-6


def make_clean_audio(sd, ds, B, T, seed, periods=PERIODS, against=None):
    """make_audio at the first of seed, seed + 1000, seed + 2000, .. whose fp64 run through discriminators `ds` has no
    pre-activation nearer to zero than MARGIN.  lrelu' jumps by 0.9 at zero, so where a pre-activation is nearer to zero than an
    fp32 forward's own error (about 1e-6 on these maps: the CPU fp32 run's deviation from fp64 is 1.1e-6 at most in the recording)
    its sign, and with it every gradient upstream, is decided by rounding: there fp32 runs differ from each other and from fp64 by
    whole terms, and no tolerance made of rounding errors means anything.  With `against` (the real audio, for the feature loss) no
    feature-map value may lie nearer than MARGIN to the one `against` gives either: |r - g| has the same kind of kink, and its
    gradient 2 / numel * sign(r - g) flips there.  The choice reads the fp64 reference alone."""
    def maps(x):
        with torch.no_grad():
            return [disc_forward(disc_params(sd, d), periods[d], x, torch.float64)[1] for d in ds]

    other = maps(against) if against is not None else None
    for n in range(400):
        x = make_audio(B, T, seed + 1000 * n)
        mine = maps(x)
        ok = all(float(torch.where(f > 0, f, f / SLOPE).abs().min()) > MARGIN for fm in mine for f in fm[:5])     # the pre-activation itself
        if ok and other is not None:
            ok = all(float((r - g).abs().min()) > MARGIN for fr, fg in zip(other, mine) for r, g in zip(fr, fg))
        if ok:
            return x
    raise RuntimeError("no seed gives a run clear of zero")


def mpd_inputs(sd, seeds, n, B, T, periods=PERIODS):
    """Case n of tests/golden/hifigan_disc.npz from its seeds: (y, y_hat, per discriminator the upstream weights of the real and of the generated side)."""
    ds = range(len(periods))
    y, y_hat = make_clean_audio(sd, ds, B, T, seeds["y"] + n), make_clean_audio(sd, ds, B, T, seeds["y_hat"] + n)
    ups = [(make_upstream(p, B, T, seeds["upstream"] + n + 10 * d), make_upstream(p, B, T, seeds["upstream"] + n + 10 * d + 5))
           for d, p in enumerate(periods)]
    return y, y_hat, ups


def mpd_total(outs, ups):
    """weighted_sum over every discriminator, real and generated side, of the four lists MultiPeriodDiscriminator returns."""
    s_r, s_g, f_r, f_g = outs
    return sum(weighted_sum(s_r[d], f_r[d], ups[d][0]) + weighted_sum(s_g[d], f_g[d], ups[d][1]) for d in range(len(ups)))


def autograd(sd, y, y_hat, dtype, loss_fn, wrt_params=True):
    """Gradients of loss_fn(the four lists) over mpd_forward: ({key: grad} over the parameters (if asked), "y" and "y_hat" where they
    reach the loss, the loss, the four lists detached)."""
    leaves = {k: v.to(dtype).clone().requires_grad_(wrt_params) for k, v in sd.items()}
    yl, hl = y.to(dtype).clone().requires_grad_(True), y_hat.to(dtype).clone().requires_grad_(True)
    outs = mpd_forward(leaves, yl, hl, dtype)
    loss = loss_fn(outs)
    loss.backward()
    g = {k: v.grad for k, v in leaves.items()} if wrt_params else {}
    g["y"], g["y_hat"] = yl.grad, hl.grad
    detached = tuple([[f.detach() for f in x] if isinstance(x, list) else x.detach() for x in part] for part in outs)
    return g, float(loss.detach()), detached


def generator_side_loss(outs):
    """The reference's feature_loss + generator_loss (hifigan_model.py:250-256, :273-281) of the four lists."""
    s_r, s_g, f_r, f_g = outs
    feat = sum((r - g).abs().mean() for dr, dg in zip(f_r, f_g) for r, g in zip(dr, dg)) * 2
    return feat + sum(((1 - g) ** 2).mean() for g in s_g)


def discriminator_side_loss(outs):
    s_r, s_g, _, _ = outs
    return sum(((1 - r) ** 2).mean() + (g ** 2).mean() for r, g in zip(s_r, s_g))
