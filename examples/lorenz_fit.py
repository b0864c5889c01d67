#!/usr/bin/env python3
"""BASELINE.json configs[0]: one trial of a Lorenz system, d_z = 3, d_y = 10, Gaussian likelihood -- the counterpart of the
reference's `script/example.py:12-47` (which fits a 2-D limit cycle the same way): make_model -> fit -> forecast.

    python examples/lorenz_fit.py [--epochs 20] [--T 1000] [--ensemble 64] [--lyapunov 10000] [--fixed-points 64] [--smooth] [--sample 64] [--score 16] [--ekf] [--laplace] [--plot out.png]

With --ensemble S it also forecasts with uncertainty: S sampled roll-outs from the last posterior (`forecast_ensemble`), the mean and
the +-2 sd band of the first latent at a few steps.  With --lyapunov N it prints the Lyapunov spectrum of the learned flow over N steps
from the last posterior mean (`lyapunov`) and the moduli of the Jacobian's eigenvalues there (`jacobian`).  With --fixed-points N it
searches for the fixed points of the learned flow from N of the filtered posterior means (`fixed_points`) and prints each distinct one,
its residual, the moduli of the eigenvalues of the Jacobian there and whether it is stable.  With --smooth it smooths the filtered
sequence with the learned dynamics (`smooth`) and prints how far the smoothed means lie from the filtered ones and the mean filtered
against the mean smoothed variance.  With --sample S it draws S whole trajectories from the smoothed posterior (`sample_posterior`)
and prints, per latent dimension, the RMS of the draws' standard deviation against the smoothed one, the lag-one correlation of the
draws, and the width of the band that holds 90 % of whole trajectories against the +-1.64 sd band of the marginals.  With --score K it
scores the learned dynamics (`score_forecast`): per horizon h = 1 .. K the R^2 of the h-step-ahead prediction of the latent state and of
the observations over the record, and the skill against persistence.  With --ekf it runs the model's own extended Kalman filter over
the record (`ekf`) and prints the evidence per row and the RMS distance between the recognition network's and the filter's means.
With --laplace it draws spike counts from the fitted read-out (a Poisson twin of the model: the learned flow and state noise, the decoder
scaled to rates of a few counts per row) and runs the Poisson filter over them (`laplace_filter`): the evidence per row, the largest
gradient norm the Newton steps left, and how far the modes lie from the trajectory the counts were drawn at.

Needs an MI355X (the filtering step runs as HIP kernels); `tests/test_host_cpu.py::test_lorenz_example_plumbing` runs the same
script against the oracle-backed stand-in on the CPU."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--n-rbf", type=int, default=100)
    ap.add_argument("--forecast", type=int, default=200)
    ap.add_argument("--ensemble", type=int, default=0, help="members of the forecast with uncertainty (0: skip it), e.g. 64")
    ap.add_argument("--lyapunov", type=int, default=0, help="steps of the Lyapunov spectrum of the learned flow (0: skip it), e.g. 10000")
    ap.add_argument("--fixed-points", type=int, default=0, help="starts of the search for fixed points of the learned flow (0: skip it), e.g. 64")
    ap.add_argument("--smooth", action="store_true", help="smooth the filtered sequence with the learned dynamics")
    ap.add_argument("--sample", type=int, default=0, help="joint draws from the smoothed posterior (0: skip them), e.g. 64")
    ap.add_argument("--score", type=int, default=0, help="horizons of the k-step-ahead prediction error over the record (0: skip it), e.g. 16")
    ap.add_argument("--ekf", action="store_true", help="the model's own extended Kalman filter over the record: evidence and means")
    ap.add_argument("--laplace", action="store_true", help="counts drawn from the fitted read-out and the Poisson filter over them: evidence per row")
    ap.add_argument("--plot", default=None)
    a = ap.parse_args(argv)
    import vjf_amd
    from vjf_amd.data import lorenz, observe

    torch.manual_seed(0)
    xdim, ydim, udim = 3, 10, 0
    g = torch.Generator().manual_seed(1)
    x = lorenz(a.T, generator=g, noise=0.05).to(torch.get_default_dtype())          # (time, 3)
    y, C, d = observe(x, ydim, "gaussian", generator=g)                              # (time, 10)

    model = vjf_amd.VJF.make_model(ydim, xdim, udim=udim, n_rbf=a.n_rbf, hidden_sizes=[20], likelihood="gaussian")
    t0 = time.perf_counter()
    m, logvar, loss = model.fit(y, max_iter=a.epochs)                                # posterior means / log-variances, last epoch's loss
    dt = time.perf_counter() - t0
    q_last = vjf_amd.Gaussian(m[-1].detach(), logvar[-1].detach())                   # the last posterior, (1, 3) each
    m = m.detach().cpu().squeeze(1)
    print(f"fit: {a.epochs} epochs x {a.T} steps in {dt:.2f} s  ({a.epochs * a.T / dt:.0f} trial-timesteps/s), final epoch loss {float(loss):.4f}")
    xf, yf = model.forecast(x0=m[9:10], n_step=a.forecast, noise=False)              # (vjf/model.py:321-324)
    print("forecast:", tuple(xf.shape), tuple(yf.shape), "finite:", bool(torch.isfinite(xf).all() and torch.isfinite(yf).all()))
    if a.ensemble > 0:
        # forecast with uncertainty: sampled roll-outs from the last posterior in one native call, their mean and +-2 sd band
        fe = model.forecast_ensemble(q_last, n_step=a.forecast, n_sample=a.ensemble, noise=True)
        mean, sd = fe.x_mean[:, 0, 0].cpu(), fe.x_var[:, 0, 0].sqrt().cpu()
        for t in sorted({0, a.forecast // 4, a.forecast // 2, a.forecast}):
            print(f"ensemble forecast: step {t:4d}  x1 = {float(mean[t]):+.3f}  [{float(mean[t] - 2 * sd[t]):+.3f}, {float(mean[t] + 2 * sd[t]):+.3f}]")
    if a.lyapunov > 0:
        # the geometry of the learned flow: its Lyapunov spectrum from the last posterior mean, the whole horizon in one native call
        # (per step of the model; in Gram-Schmidt column order, which a long horizon sorts), and the Jacobian's eigenvalues there
        ly = model.lyapunov(q_last, n_step=a.lyapunov, burn_in=min(1000, a.lyapunov))
        print(f"lyapunov: {a.lyapunov} steps  exponents per step = {[round(float(v), 5) for v in ly.exponents[0].cpu()]}"
              f"  sum = {float(ly.exponents[0].sum()):+.5f}")
        ev = torch.linalg.eigvals(model.jacobian(q_last)[0].cpu())
        print("jacobian at the last posterior mean: |eigenvalues| =", [round(float(v), 4) for v in ev.abs()])
    if a.fixed_points > 0:
        # where the learned flow stands still, and whether it stays there: N starts drawn from the filtered posterior means, the whole
        # damped Newton search of every start in one native call; a fixed point is stable if every eigenvalue of the Jacobian of the
        # map lies inside the unit circle
        rows = torch.randint(0, m.shape[0], (a.fixed_points,), generator=torch.Generator().manual_seed(2))
        fp = model.fixed_points(m[rows])
        ux, uj, count = fp.unique()
        print(f"fixed points: {int(fp.converged.sum())} of {a.fixed_points} starts converged, {len(ux)} distinct")
        for xk, jk, ck in zip(ux.cpu(), uj.cpu(), count):
            near = ((fp.x.cpu() - xk).norm(dim=1) <= 1e-3) & fp.converged.cpu()
            mod = torch.linalg.eigvals(jk).abs()
            print(f"  x = {[round(float(v), 4) for v in xk]}  residual = {float(fp.residual.cpu()[near].max()):.2e}  reached by {int(ck)}"
                  f"  |eigenvalues| = {[round(float(v), 4) for v in mod]}  {'stable' if bool((mod < 1).all()) else 'unstable'}")
    if a.smooth:
        # the latent trajectory given the whole record, q(x_t | y_1..T): the extended Rauch-Tung-Striebel pass over the filtered
        # posterior in one native call, the state noise being the transition's own
        sm = model.smooth((m, logvar.detach()))
        rms = float((sm.mean.cpu()[:, 0] - m).pow(2).sum(-1).mean().sqrt())
        print(f"smooth: RMS |smoothed - filtered mean| = {rms:.4f}   mean variance filtered {float(logvar.detach().exp().mean()):.3e}"
              f" -> smoothed {float(sm.var.mean()):.3e}")
    if a.sample > 0:
        # whole trajectories from the smoothed posterior: backward sampling in one native call.  Their spread per row is the smoother's;
        # what they add is how rows co-vary -- a band that holds 90 % of whole paths is wider than the marginals' +-1.64 sd
        q = (m, logvar.detach())
        sm = model.smooth(q)
        xs = model.sample_posterior(q, n_sample=a.sample).x[:, :, 0].cpu()              # (S, T, 3)
        mean, sd = sm.mean[:, 0].cpu(), sm.var[:, 0].sqrt().cpu()
        dev = (xs - mean) / sd                                                          # standardised deviations of the draws
        reach = dev.abs().amax(dim=1)                                                   # (S, 3): the farthest a path strays, in sd
        for k in range(xdim):
            rms = float((xs[..., k].std(dim=0) / sd[:, k] - 1).pow(2).mean().sqrt()) if a.sample > 1 else float("nan")
            lag = float((dev[:, 1:, k] * dev[:, :-1, k]).mean())
            print(f"sample: x{k + 1}  RMS relative error of the draws' sd against the smoothed sd = {rms:.3f}   lag-one correlation = {lag:+.3f}"
                  f"   90 % of whole paths stay within +-{float(reach[:, k].quantile(0.9)):.2f} sd (marginal band: +-1.64 sd)")
    if a.score > 0:
        # how good the learned dynamics are: from every row of the filtered record the mean map rolled h = 1 .. K steps, against what the
        # filter found and what was observed h rows on, the whole record in one native call
        sc = model.score_forecast(m, y, n_step=a.score)
        r2x, r2y, skx, sky = (v.cpu() for v in (sc.r2_x(), sc.r2_y(), sc.skill_x(), sc.skill_y()))
        for h in range(1, a.score + 1):
            print(f"score: h = {h:3d}  n = {int(sc.n[h]):6d}  R2 x = {float(r2x[h]):+.4f}  y = {float(r2y[h]):+.4f}"
                  f"   skill against persistence x = {float(skx[h]):+.4f}  y = {float(sky[h]):+.4f}")
    if a.ekf:
        # the model's own Bayesian filter, no recognition network: the extended Kalman filter of the learned flow, state noise, decoder
        # and observation noise over the whole record in one native call -- the evidence log p(y_t | y_1..t-1) row by row, and how far
        # the amortised posterior means lie from it
        ek = model.ekf(y)
        rms = float((ek.mean.cpu()[:, 0] - m).pow(2).sum(-1).mean().sqrt())
        print(f"ekf: evidence per row = {float(ek.log_likelihood()[0]) / a.T:+.4f}   RMS |recognition - ekf mean| = {rms:.4f}"
              f"   mean variance recognition {float(logvar.detach().exp().mean()):.3e} -> ekf {float(ek.var.mean()):.3e}")
    if a.laplace:
        # the same for spike counts: a Poisson twin with the fitted flow, state noise and read-out (scaled so that the log rates stay
        # within +-2), counts drawn at the filtered means, and the model's own filter over them -- the Laplace evidence row by row
        pm = vjf_amd.VJF.make_model(ydim, xdim, udim=udim, n_rbf=a.n_rbf, hidden_sizes=[20], likelihood="poisson")
        for dst, src in ((pm.transition.velocity.feature.centroid, model.transition.velocity.feature.centroid),
                         (pm.transition.velocity.feature.logwidth, model.transition.velocity.feature.logwidth),
                         (pm.transition.velocity.w_mean, model.transition.velocity.w_mean), (pm.transition.logvar, model.transition.logvar)):
            dst.copy_(src)
        eta = model.decoder(m.to(model.decoder.decode.weight.device))
        gain = 2.0 / float(eta.abs().max().clamp(min=2.0))
        pm.decoder.decode.weight.copy_(gain * model.decoder.decode.weight)
        pm.decoder.decode.bias.copy_(gain * model.decoder.decode.bias)
        counts = torch.poisson((gain * eta).exp().cpu(), generator=torch.Generator().manual_seed(3)).to(eta.device)
        lf = pm.laplace_filter(counts, x0=vjf_amd.Gaussian(m[:1].to(eta.device), logvar[0].detach().to(eta.device)))
        rms = float((lf.mean.cpu()[:, 0] - m).pow(2).sum(-1).mean().sqrt())
        print(f"laplace_filter: mean count {float(counts.mean()):.2f}   evidence per row = {float(lf.log_likelihood()[0]) / a.T:+.4f}"
              f"   largest grad_norm = {float(lf.grad_norm.max()):.2e}   RMS |mode - trajectory| = {rms:.4f}")
    if a.plot:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        fig, ax = plt.subplots(1, 3, figsize=(12, 3))
        ax[0].plot(x.numpy()); ax[0].set_title("True state")
        ax[1].plot(m.numpy()); ax[1].set_title("Posterior mean")
        ax[2].plot(xf.detach().cpu().squeeze(1).numpy()); ax[2].set_title("Forecast")
        fig.tight_layout(); fig.savefig(a.plot)
    return m, loss


if __name__ == "__main__":
    main()
