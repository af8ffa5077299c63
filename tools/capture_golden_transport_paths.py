#!/usr/bin/env python
"""Generates tests/golden/transport_paths_<path>_<prediction>.npz by running the reference's own `diffusion.transport` package (read from the reference checkout
oracle/capture_golden.py points at) on the CPU in f32 with a noise- or a score-predicting model: the small LightningDiT of oracle/capture_golden_sampler.py
(same `DIT_KW`, `DIT_SEED`, z, y and time shift), whose output the transport reads as the noise / the score.  Per (path, prediction) pair the fixture holds

  coeffs      [10, 7]: t, alpha, d_alpha, sigma, d_sigma, d_alpha / alpha, drift_var of the path at ten times,
  intervals   the whole `check_interval` table of the pair's transport,
  t, x0, pred, loss   `Transport.sample` / `training_losses` on x1 under the recorded seed,
  xs_euler    `sample_sde` Euler / sigma / "Mean" / 0.04 / 6 steps, seed 11,
  xs_heun     `sample_sde` Heun / linear, norm 0.7 / "Tweedie" / 0.05 / 5 steps, seed 11,

for the eight (path, prediction) pairs other than Linear / velocity, with eps passed explicitly: VP (1e-5, 1e-3), velocity on GVP (0, 0), noise / score on
Linear / GVP (1e-3, 1e-3).  Every captured tensor is asserted finite.  The fixtures hold tensors, seeds and settings only.

Run:  TORCHDYNAMO_DISABLE=1 python tools/capture_golden_transport_paths.py        (CPU, seconds)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import capture_golden as cg  # noqa: E402
from oracle.capture_golden_sampler import DIT_KW, DIT_SEED  # noqa: E402
from oracle.detweights import det_fill_  # noqa: E402

PAIRS = (("Linear", "noise", 1e-3, 1e-3), ("Linear", "score", 1e-3, 1e-3),
         ("GVP", "velocity", 0, 0), ("GVP", "noise", 1e-3, 1e-3), ("GVP", "score", 1e-3, 1e-3),
         ("VP", "velocity", 1e-5, 1e-3), ("VP", "noise", 1e-5, 1e-3), ("VP", "score", 1e-5, 1e-3))
TIMES = (1e-3, 0.05, 0.2, 0.35, 0.5139, 0.65, 0.8, 0.9, 0.96, 0.999)
SHIFT = 2.5
SDE_CASES = {"euler": dict(sampling_method="Euler", diffusion_form="sigma", diffusion_norm=1.0, last_step="Mean", last_step_size=0.04, num_steps=6),
             "heun": dict(sampling_method="Heun", diffusion_form="linear", diffusion_norm=0.7, last_step="Tweedie", last_step_size=0.05, num_steps=5)}
SDE_SEED, TRAIN_SEED = 11, 21


def fixture_name(path, prediction):
    return f"transport_paths_{path.lower()}_{prediction}"


def main():
    cg.install_stubs()
    torch.set_grad_enabled(False)
    from diffusion.lightningdit.lightningdit import LightningDiT
    from diffusion.transport import Sampler, create_transport
    m = det_fill_(LightningDiT(**DIT_KW).eval(), DIT_SEED, skip=("pos_embed",))
    g = torch.Generator().manual_seed(4242)
    z = torch.randn(4, 8, 8, 8, generator=g)
    x1 = torch.randn(4, 8, 8, 8, generator=g)
    y = torch.tensor([3, 0, 9, 10])
    for path, prediction, train_eps, sample_eps in PAIRS:
        tr = create_transport(path, prediction, None, train_eps, sample_eps, time_dist_shift=SHIFT)
        assert (tr.train_eps, tr.sample_eps) == (train_eps, sample_eps)
        ps = tr.path_sampler
        t = torch.tensor(TIMES, dtype=torch.float32)
        te = t.view(-1, 1)
        alpha, d_alpha = ps.compute_alpha_t(te)
        sigma, d_sigma = ps.compute_sigma_t(te)
        full = lambda v: v.expand_as(te) if torch.is_tensor(v) else torch.full_like(te, float(v))
        coeffs = torch.cat([te, full(alpha), full(d_alpha), full(sigma), full(d_sigma), full(ps.compute_d_alpha_alpha_ratio_t(te)),
                            full(ps.compute_drift(torch.ones_like(te), t)[1])], dim=1)
        rows = []
        for form in ("SBDM", "sigma"):
            for sde in (False, True):
                for ev in (False, True):
                    for rev in (False, True):
                        for lss in (0.0, 0.04):
                            t0, t1 = tr.check_interval(tr.train_eps, tr.sample_eps, diffusion_form=form, sde=sde, eval=ev, reverse=rev, last_step_size=lss)
                            rows.append([form == "SBDM", sde, ev, rev, lss, t0, t1])
        torch.manual_seed(TRAIN_SEED)
        tt, terms = tr.training_losses(m, x1, dict(y=y))
        torch.manual_seed(TRAIN_SEED)
        t2, x0, _ = tr.sample(x1)
        assert torch.equal(tt, t2)
        out = dict(coeffs=coeffs, intervals=np.array(rows, dtype=np.float64), t=tt, x0=x0, pred=terms["pred"], loss=terms["loss"])
        sampler = Sampler(tr)
        for tag, kw in SDE_CASES.items():
            torch.manual_seed(SDE_SEED)
            out[f"xs_{tag}"] = torch.stack(sampler.sample_sde(**kw)(z, m.forward, y=y))
            for k, v in kw.items():
                out[f"{tag}_{k}"] = np.array(v)
        for k, v in out.items():
            if torch.is_tensor(v):
                assert torch.isfinite(v).all(), (path, prediction, k)
                print(f"  {path}/{prediction} {k}: max |.| {v.abs().max().item():.4g}")
        cg.save(fixture_name(path, prediction), path=np.array(path), prediction=np.array(prediction), train_eps=np.array(train_eps), sample_eps=np.array(sample_eps),
                time_dist_shift=np.array(SHIFT), dit_seed=np.array(DIT_SEED), sde_seed=np.array(SDE_SEED), train_seed=np.array(TRAIN_SEED), z=z, x1=x1, y=y, **out)


if __name__ == "__main__":
    main()
