"""Differential-evolution moves on the GPU: the kernel against the host build of phf_hier_de.h bit for bit (theta, log-target, trace,
statistics), the independence of populations, the sampler integration (cuts, fused launch, checkpoint, K = 0), the posterior against
golden G11 and the command line."""
import glob
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from test_de_moves_host import _same_bits, build_shim, experiments_of, packed_pair, twin_round

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("hier_de_gpu"))


def _sampler(gpu, ne, Q, C, seed=25, problem_ids=None, chain_id_base=0, thinning=5):
    """Q problems (the synthetic pairs 0..Q-1 at ne experiments) x C chains, started at the sampler's own start points"""
    from pyhillfit_amd import bestfit
    from pyhillfit_amd import hierarchical as H
    exs = [experiments_of(ne, q) for q in range(Q)]
    s = H.HierarchicalSampler(H.PackedHierPoints(exs), list(range(Q)), C, thinning=thinning, seed=seed, problem_ids=problem_ids,
                              chain_id_base=chain_id_base, device=gpu)
    s.init(np.array(bestfit.hierarchical_first_iteration_batch(exs, H.prior_params()[2])), cov_scale=0.01)
    return s, exs


# ---- 1. the kernel against the host build ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ne,Q,C,G", [(1, 1, 64, 64), (3, 1, 64, 4), (4, 1, 64, 64), (9, 1, 64, 4), (3, 2, 128, 64), (9, 2, 128, 16),
                                      (1, 2, 128, 8)])
def test_kernel_against_host_build(gpu, shim, ne, Q, C, G):
    """states that 200 real iterations produced; one ordinary round and one gamma = 1 round, each compared with the twin: the whole
    state (theta and log-target moved, nothing else touched), the trace, the statistics"""
    ids, base, seed = [5, 9][:Q], 128, 25 | (3 << 32)
    s, exs = _sampler(gpu, ne, Q, C, seed=seed, problem_ids=ids, chain_id_base=base)
    s.advance(200, save=False)
    de = s.enable_de_moves(100, population=G, jump_every=10)
    pairs = [packed_pair(e) for e in exs]
    dim, nch = s.d, Q * C
    want = s.state.cpu().numpy().copy()
    want_att, want_acc = np.zeros((2, Q), dtype=np.int64), np.zeros((2, Q), dtype=np.int64)
    for rnd in (3, 10):
        kind = int(rnd % 10 == 0)
        gamma = de.gamma_of(rnd)
        assert gamma == (1.0 if kind else 2.38 / np.sqrt(2.0 * dim))
        trace = torch.full((Q, C, 6), float("nan"), dtype=torch.float64, device=gpu)
        de.round(rnd, trace=trace)
        got = s.state.cpu().numpy()
        want_trace = np.empty((Q, C, 6))
        for q in range(Q):
            tr, att, acc, _ = twin_round(shim, pairs[q], G, base, ids[q], rnd, seed, gamma, want[:dim, q * C:(q + 1) * C],
                                         want[dim, q * C:(q + 1) * C], ts=nch, chains=C)
            want_trace[q] = tr
            want_att[kind, q] += att; want_acc[kind, q] += acc
        assert _same_bits(trace.cpu().numpy(), want_trace), rnd
        assert _same_bits(got, want), rnd
        st = de.statistics()
        assert np.array_equal(st["attempts"], want_att[0]) and np.array_equal(st["accepts"], want_acc[0])
        assert np.array_equal(st["jump_attempts"], want_att[1]) and np.array_equal(st["jump_accepts"], want_acc[1])
    print("Ne=%d Q=%d C=%d G=%d: accepted %s of %s (ordinary), %s of %s (gamma = 1)"
          % (ne, Q, C, G, want_acc[0].sum(), want_att[0].sum(), want_acc[1].sum(), want_att[1].sum()))
    # some move was accepted, so the write of theta and log-target was compared (after 200 iterations the chains of a pair still sit
    # close together: at Ne = 9 every ordinary proposal is accepted; the rejections are in the rounds of the smaller models)
    assert np.all(want_att == C) and want_acc.sum() > 0
    assert de.rounds == 2


# ---- 2. populations do not interact ---------------------------------------------------------------------------------------------------
def test_populations_are_independent(gpu):
    s, _ = _sampler(gpu, 3, 2, 64)
    s.advance(200, save=False)
    de = s.enable_de_moves(100, population=8)
    start = s.state.clone()
    de.round(2)
    plain = s.state.clone()
    s.state.copy_(start)
    cols = torch.arange(64 + 16, 64 + 24, device=gpu)                            # population 2 of problem 1
    s.state[:s.d, cols] *= 1.01
    de.round(2)
    other = torch.ones(128, dtype=torch.bool, device=gpu)
    other[cols] = False
    assert torch.equal(s.state[:, other], plain[:, other])
    assert not torch.equal(s.state[:s.d, cols], plain[:s.d, cols])


# ---- 3. the sampler integration -------------------------------------------------------------------------------------------------------
def test_sampler_integration(gpu):
    """2 pairs x 64 chains, Ne = 3, 2 000 iterations, K = 100: rows and final state do not depend on how the run is cut, on the fused
    launch or on a checkpoint in the middle; K = 0 is the sampler without the feature"""
    from pyhillfit_amd import hierarchical as H

    def make(every):
        s, _ = _sampler(gpu, 3, 2, 64)
        if every is not None:
            s.enable_de_moves(every)
        return s

    def run(s, cuts, adv=None):
        rows = torch.cat([s.advance(k) if adv is None else adv(k)[0] for k in cuts])
        return rows, s.state.clone()

    never = make(None)
    rows_never, state_never = run(never, [2000])
    off = make(0)
    assert off.de is None
    rows_off, state_off = run(off, [2000])
    assert torch.equal(rows_off, rows_never) and torch.equal(state_off, state_never)

    one = make(100)
    rows, state = run(one, [2000])
    assert rows.shape == (400, 2, 12, 64) and one.de.rounds == 20 and one.t == 2000
    assert not torch.equal(rows, rows_never)                                     # the moves did move chains
    st = one.de.statistics()
    assert st["attempts"].tolist() == [18 * 64] * 2 and st["jump_attempts"].tolist() == [2 * 64] * 2
    assert all(0 < a < 18 * 64 for a in st["accepts"])
    for cuts in ([100] * 20, [300, 700, 1000], [250, 450, 1300], [5, 95, 1900]):
        s = make(100)
        r2, s2 = run(s, cuts)
        assert torch.equal(r2, rows) and torch.equal(s2, state), cuts
        assert s.de.rounds == 20
    # the fused launch
    s = make(100)
    f = H.FusedSamplers([s])
    r2, s2 = run(s, [600, 1400], adv=f.advance)
    f.check_queue()
    assert torch.equal(r2, rows) and torch.equal(s2, state) and s.de.rounds == 20
    # a checkpoint in the middle
    s = make(100)
    first = s.advance(1000)
    sd = s.state_dict()
    t = make(100)
    t.load_state_dict(sd)
    second = t.advance(1000)
    assert torch.equal(torch.cat([first, second]), rows) and torch.equal(t.state, state)
    # refusals
    with pytest.raises(ValueError, match="multiple of the thinning"):
        make(None).enable_de_moves(102)
    with pytest.raises(ValueError, match="population"):
        make(None).enable_de_moves(100, population=48)


# ---- 4. the posterior -----------------------------------------------------------------------------------------------------------------
def test_g11_one_experiment_posteriors_with_moves(gpu):
    """The Ne = 1 entries of golden G11 by the recipe of _hier_posteriors_against_reference_loop (tests/test_gpu_hierarchical.py): 512 chains
    from the fixture's start point, the fixture's run length and burn-in, moments on the device — with the moves on, K = 100, G = 64.  That
    function's bars: every column's pooled mean within 1 % + 4 standard errors of the reference's, every pooled sd within its band
    [max(0.5, 0.8 - 4 r), min(3, 1.2 + 4 r)] of the reference's pooled sd.  (Only the Ne = 1 entries: the run is to stay within seconds.)"""
    from pyhillfit_amd import doseresponse as dr
    from pyhillfit_amd import hierarchical as H
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    with open(os.path.join(GOLDEN, "g11_hier_posteriors_few_experiments.json")) as f:
        entries = [e for e in json.load(f) if e["Ne"] == 1]
    assert len(entries) == 4
    T, thin = entries[0]["iterations"], entries[0]["thinning"]
    assert all(e["iterations"] == T and e["thinning"] == thin for e in entries) and T >= 300000
    exs = [dr.load_crumb_data(e["drug"], e["channel"])[2][:1] for e in entries]
    s = H.HierarchicalSampler(H.PackedHierPoints(exs), list(range(len(exs))), 512, thinning=thin, seed=2029, device=gpu)
    s.init(np.array([e["first_iteration"] for e in entries]), cov_scale=0.01)
    burn_rows = (T // thin + 1) // 4
    s.enable_moments(after_iteration=burn_rows * thin - 1)
    s.enable_de_moves(100, population=64)
    for _ in range(10):
        s.advance(T // 10, save=False)
    mean, var, n = s.posterior_moments()
    assert n == T // thin + 1 - burn_rows and s.de.rounds == T // 100
    pooled = mean.mean(dim=2).cpu().numpy()
    pooled_sd = torch.sqrt(var.mean(dim=2) + mean.var(dim=2)).cpu().numpy()
    acc = s.acceptance().mean(dim=1).cpu().numpy()
    recs = s.de.records()
    bad = []
    for q, e in enumerate(entries):
        p = e["pooled"]
        want, want_sd = np.array(p["mean"]), np.array(p["sd"])
        se = np.maximum(p["se_batch_means"], p["se_between_seeds"])
        ratio = np.abs(pooled[:, q] - want) / (0.01 * np.abs(want) + 4 * se)
        sd_ratio = pooled_sd[:, q] / want_sd
        run_means = np.array([r["mean"] for r in e["runs"]]); run_sds = np.array([r["sd"] for r in e["runs"]])
        v_seed = run_sds ** 2 + (run_means - run_means.mean(axis=0)) ** 2
        rel_se_sd = v_seed.std(axis=0, ddof=1) / np.sqrt(len(e["runs"])) / (2.0 * np.maximum(v_seed.mean(axis=0), 1e-300))
        sd_lo, sd_hi = np.maximum(0.5, 0.8 - 4 * rel_se_sd), np.minimum(3.0, 1.2 + 4 * rel_se_sd)
        print("de-moves g11 %s-%s Ne=1: worst mean ratio %.2f (column %d), sd ratios %.3f..%.3f, acceptance %.3f, move accept rates %.3f / %.3f"
              % (e["drug"], e["channel"], ratio.max(), int(ratio.argmax()), sd_ratio.min(), sd_ratio.max(), acc[q], recs[q]["accept_rate"],
                 recs[q]["jump_accept_rate"]))
        if not ratio.max() < 1.0:
            bad.append((e["drug"], e["channel"], "mean of column %d: ratio %.2f" % (int(ratio.argmax()), ratio.max())))
        if not (np.all(sd_ratio > sd_lo) and np.all(sd_ratio < sd_hi)):
            bad.append((e["drug"], e["channel"], "sd ratios %.3f..%.3f" % (sd_ratio.min(), sd_ratio.max())))
    assert not bad, bad


# ---- 5. the command line ---------------------------------------------------------------------------------------------------------------
def test_command_line(gpu, tmp_path, capsys):
    from pyhillfit_amd import PyHillFit
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    csv = tmp_path / "crumb_data.csv"
    dr.table.to_csv(str(csv))
    PyHillFit.main(["--data-file", str(csv), "-m", "2", "--hierarchical", "-i", "4000", "--drugs", "Amiodarone,Bepridil", "--channels", "hERG",
                    "--num-chains", "64", "--segment", "1500", "--de-every", "100", "--diagnostics", "--output-root", str(tmp_path / "out")])
    text = capsys.readouterr().out
    assert "de-moves [rank 0]: every 100 iterations, populations of 64, 40 rounds; lowest accept rate" in text
    assert "coupled within populations of 64" in text
    files = sorted(glob.glob(os.path.join(str(tmp_path / "out"), "**", "*_summary.json"), recursive=True))
    assert len(files) == 2
    for p in files:
        with open(p) as f:
            summ = json.load(f)
        rec = summ["de_moves"]
        assert (rec["every"], rec["population"], rec["jump_every"], rec["rounds"]) == (100, 64, 10, 40)
        assert rec["gamma"] == 2.38 / np.sqrt(2.0 * (5 + 2 * summ["num_expts"]))
        assert rec["attempts"] == 36 * 64 and rec["jump_attempts"] == 4 * 64
        assert 0.0 < rec["accept_rate"] < 1.0 and 0.0 < rec["jump_accept_rate"] < 1.0
        assert summ["diagnostics"]["chains_coupled_within_populations_of"] == 64
        chain = np.loadtxt(p.replace("_summary.json", ".txt"))
        assert chain.shape == (4000 // 5 + 1, 5 + 2 * summ["num_expts"] + 1) and np.isfinite(chain).all()
