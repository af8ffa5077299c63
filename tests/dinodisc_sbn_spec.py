"""The DINOv2 discriminator in the configuration the reference's trainers build (train_tokenizer.py:307-314, train_dmd.py:389-396: `norm_type="sbn"`,
`use_specnorm=False`, models/dinodisc.py:62-65) restated over plain parameter dicts, on top of tests/dinodisc_spec.py (backbone, preprocessing, name-seeded fill).

SyncBatchNorm is stated by its formulas, not through `nn.SyncBatchNorm`, on [B, C, L]:
  train   mean[c] = sum x / N, var[c] = sum (x - mean)^2 / N over all B * L positions of all ranks (N = the global count; `reduce` sums a tensor over the ranks,
          identity in a single process; the sums in float64); y = (x - mean) / sqrt(var + eps) * weight + bias, evaluated as x alpha + beta with
          alpha = weight / sqrt(var + eps), beta = bias - mean alpha -- LeakyReLU's derivative jumps at zero, and an f32 statement that rounds a pre-activation
          differently from the reference takes the other side for one element in a million, which moves single gradient entries by 1e-3 of the largest
          (tests/dinodisc_spec.py); running_mean <- 0.9 running_mean + 0.1 mean,
          running_var <- 0.9 running_var + 0.1 var N / (N - 1), num_batches_tracked += 1 (returned in `new_state`, the dict passed in is not written)
  eval    the same map with mean = running_mean, var = running_var
then LeakyReLU(0.2).

bf16 sites (q = oracle.ref_cpu.bf16_round), beyond the backbone's and the tap's (tests/dinodisc_spec.py):
  train   as the 'bn' heads: conv result q(.), norm + LeakyReLU result q(.), the f32 tail unrounded
  eval    the HIP route folds norm + LeakyReLU into the convolution's epilogue: the conv result is never stored, so only a = q(.) and h = q(.) round forward;
          backward, the gradient at the conv result is still a stored bf16 tensor (the operand of the input-gradient conv): rounded there, gradient only."""
import math

import torch
import torch.nn.functional as F

import dinodisc_spec as S
from oracle import ref_cpu as R
from oracle.detweights import det_tensor

SMALL = dict(ks=9, key_depths=(0, 3), depth=4, batch=12, px=256, seed=46, x_seed=5, dy_seed=6, norm_eps=1e-6)      # tests/golden/dinodisc_sbn_small.npz
# seed 46: of the seeds 37 ... 60 the one whose closest pre-activation to LeakyReLU's kink, in the reference's own f32 runs, is farthest from it (3.6e-7;
# tools/capture_golden_dinodisc_sbn.py --pick-seed) -- with seed 37 one element sat 1.9e-8 from zero and the capture itself took the other side from a float64 run.
MOMENTUM = 0.1
TRACKED0 = 3                  # num_batches_tracked before the captured calls


def filled_heads(shapes: dict, seed: int) -> dict:
    """`dinodisc_spec.filled_heads` for a state_dict with SyncBatchNorm heads: running_var moved to 0.5 + |x| (positive), num_batches_tracked an int64 scalar."""
    out = S.filled_heads({k: s for k, s in shapes.items() if not k.endswith("num_batches_tracked")}, seed)
    for k, shp in shapes.items():
        if not k.startswith("heads."):
            continue
        if k.endswith("running_var"):
            out[k] = 0.5 + det_tensor(k, tuple(shp), seed).abs()
        elif k.endswith("num_batches_tracked"):
            out[k] = torch.tensor(TRACKED0, dtype=torch.int64)
    return {k: out[k] for k in shapes if k in out}


class _RoundGradOnly(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def sync_batchnorm(x, p, pre, train, eps, new_state=None, reduce=None):
    """x [B, C, L] -> the normalised, affine-mapped x (no activation).  `reduce`: a differentiable sum over the ranks (None: one rank)."""
    red = (lambda v: v) if reduce is None else reduce
    if train:
        xd = x.double()                                   # the sums in float64, as ATen's CPU batch_norm accumulates them
        n = red(torch.tensor(float(x.shape[0] * x.shape[2]), dtype=torch.float64))
        mean = red(xd.sum((0, 2))) / n
        var = red(((xd - mean[None, :, None]) ** 2).sum((0, 2))) / n
        if new_state is not None:
            with torch.no_grad():
                new_state[pre + "running_mean"] = (1 - MOMENTUM) * p[pre + "running_mean"] + MOMENTUM * mean.to(x.dtype)
                new_state[pre + "running_var"] = (1 - MOMENTUM) * p[pre + "running_var"] + MOMENTUM * (var * (n / (n - 1))).to(x.dtype)
                new_state[pre + "num_batches_tracked"] = p[pre + "num_batches_tracked"] + 1
        mean, invstd = mean.to(x.dtype), (1 / torch.sqrt(var + eps)).to(x.dtype)
    else:
        mean, invstd = p[pre + "running_mean"], 1 / torch.sqrt(p[pre + "running_var"] + eps)
    alpha = invstd * p[pre + "weight"]                    # y = (x - mean) invstd weight + bias as one multiply-add per element: x alpha + beta
    beta = (p[pre + "bias"].double() - mean.double() * alpha.double()).to(x.dtype)
    return (x.double() * alpha.double()[None, :, None] + beta.double()[None, :, None]).to(x.dtype)      # one rounding: a fused multiply-add


def head(t, p, pre, ks, train, q=None, new_state=None, reduce=None, eps=SMALL["norm_eps"], fused_eval=True):
    """One head on the tap t [B, 1 + L, C] -> logits [B, L] (models/dinodisc.py:134-141,182-190; plain convolutions, SyncBatchNorm).  fused_eval=False: the eval
    mode of heads that train (the composed route), with the train mode's sites."""
    act = R._q(q, t[:, 1:] + t[:, :1]).transpose(1, 2)
    site = (lambda v: R._q(q, v)) if train or q is None or not fused_eval else _RoundGradOnly.apply      # the conv result: stored, or a gradient site only
    h0 = site(F.conv1d(act, R._qw(q, p[pre + "0.0.weight"]), p[pre + "0.0.bias"]))
    a = R._q(q, F.leaky_relu(sync_batchnorm(h0, p, pre + "0.1.", train, eps, new_state, reduce), 0.2))
    c1 = site(F.conv1d(a, R._qw(q, p[pre + "1.fn.0.weight"]), p[pre + "1.fn.0.bias"], padding=ks // 2))
    h = R._q(q, F.leaky_relu(sync_batchnorm(c1, p, pre + "1.fn.1.", train, eps, new_state, reduce), 0.2))
    return F.conv1d((a + h) * (1 / math.sqrt(2)), p[pre + "2.weight"], p[pre + "2.bias"]).reshape(t.shape[0], -1)


def forward(x, backbone, heads, ks=SMALL["ks"], key_depths=SMALL["key_depths"], num_heads=6, train=True, branch="area", crop=None, q=None, new_state=None,
            reduce=None, fused_eval=True):
    """Logits [B, len(key_depths) * L]; train mode: `new_state` (a dict) receives the running statistics and counters after the call."""
    taps = S.backbone_taps(S.preprocess(x, branch, crop), backbone, key_depths, num_heads, q)
    return torch.cat([head(t, heads, f"heads.{i}.", ks, train, q, new_state, reduce, fused_eval=fused_eval) for i, t in enumerate(taps)], dim=1)


def is_param(k: str) -> bool:
    return not k.endswith(("running_mean", "running_var", "num_batches_tracked"))


def build_module(device="cpu", norm_type="sbn", ks=SMALL["ks"], key_depths=SMALL["key_depths"], depth=SMALL["depth"], seed=SMALL["seed"]):
    """This build's DinoDisc in the scripts' configuration on the capture's reduced backbone, name-seeded; the caller has the SyncBatchNorm switch on.
    -> (module, backbone dict, heads dict)"""
    import warnings
    from dmvae_amd.models.dinodisc import DinoDisc
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        disc = DinoDisc(ks, "cpu", None, key_depths=key_depths, dino_depth=depth, norm_type=norm_type, norm_eps=SMALL["norm_eps"], use_specnorm=False)
    backbone = S.filled_backbone({k: v.shape for k, v in disc.dino[0].state_dict().items()}, seed)
    disc.dino[0].load_state_dict(backbone, strict=True)
    heads = filled_heads({k: v.shape for k, v in disc.state_dict().items()}, seed)
    missing, unexpected = disc.load_state_dict(heads, strict=False)
    assert set(missing) == {"x_scale", "x_shift"} and not unexpected
    return disc.to(device), backbone, heads
