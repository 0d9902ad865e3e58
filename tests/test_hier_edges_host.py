"""The edge-state scenarios of tests/hier_edge_scenarios.py on the scalar twin alone (no GPU): the conditions that keep the kernel
comparison of tests/test_gpu_isa_edges.py from being vacuous — both accept outcomes occur where they should, chains do sit at -inf and do
step inside, the frozen chains stay frozen, the zero covariance stays zero, the edited data reach the target as -inf and -69 — and the
optional per-iteration trace of PackedHierPair.advance that counts them.  The inputs are tuned against the twin, never against a kernel."""
import numpy as np
import pytest

import hier_edge_scenarios as sc


@pytest.fixture(scope="module")
def groups(oracle_pair):
    """group name -> (experiments of its three pairs, healthy starts): the seven Crumb shapes and the synthetic Ne = 1, 2, 9"""
    out = {name: ([oracle_pair(d, c).experiments for d, c in names], theta0) for name, (names, theta0) in sc.SHAPES.items()}
    out.update({name: sc.synthetic_group(name) for name in sc.SYNTHETIC})
    return out


def _locs():
    from pyhillfit_amd import hierarchical as H
    return H.prior_params()[2]


def _shares(res):
    """over the checked chains of one run: per problem (accepted, proposed), and the shares of the whole run"""
    per_problem = {}
    for (q, c), (rows, st, tr) in res.items():
        a, n = per_problem.get(q, (0, 0))
        per_problem[q] = (a + int(tr[:, 1].sum()), n + len(tr))
    tr = np.concatenate([v[2] for v in res.values()])
    lt = np.concatenate([v[0][:, -1] for v in res.values()])
    return per_problem, dict(accepted=float(tr[:, 1].mean()), bad=float(np.mean(np.isneginf(tr[:, 0]) | np.isnan(tr[:, 0]))),
                             outside=float(tr[:, 2].mean()), rows_at_minus_inf=float(np.mean(np.isneginf(lt))))


CASES = [(s, g) for s in sc.SCENARIOS for g in sc.SHAPES] + [(s, g) for s in sc.SYNTHETIC_SCENARIOS for g in sc.SYNTHETIC]


@pytest.mark.parametrize("scenario,group", CASES)
def test_scenario_on_the_twin(scenario, group, groups):
    from oracle import c_oracle as co
    experiments, theta0 = groups[group]
    dim = len(theta0[0])
    for run in sc.runs_of(scenario, theta0, _locs()):
        exs = sc.experiments_of(run, experiments)
        res = sc.twin_run(run, exs, trace=True)
        per_problem, shares = _shares(res)
        print("%s | %s | %s: accepted %.3f, proposals at -inf or NaN %.3f, outside the support %.3f, saved rows at -inf %.3f; per problem accepted %s"
              % (group, scenario, run.key, shares["accepted"], shares["bad"], shares["outside"], shares["rows_at_minus_inf"],
                 [a for a, _ in (per_problem[q] for q in sorted(per_problem))]))
        start = sc.starts(run)
        for (q, c), (rows, st, tr) in res.items():
            # the trace is the loop's own record: accept decisions sum to the state's accept count, accepted proposals are the saved targets
            assert st[-1] == tr[:, 1].sum() and tr.shape == (sc.T, 3)
            assert np.isnan(rows[:, :dim]).sum() == 0                                  # states stay finite numbers whatever the target says
            assert np.isfinite(st[:dim]).all()
        if (scenario in ("a", "b") and run.cov_scale == 1.0) or (scenario == "f" and run.cov_scale == 0.125):
            for q, (a, n) in per_problem.items():
                assert 0 < a < n, (run.key, q, a, n)                                   # both outcomes, in every problem
        if scenario == "f" and run.cov_scale == 1.0:
            # a problem whose start sits at its pair's mode accepts nothing at this scale (hier_edge_scenarios.runs_of): both outcomes
            # over the run, rejections in every problem; the run at 1/8 has both in every problem
            assert 0.0 < shares["accepted"] and all(a < n for a, n in per_problem.values()), (run.key, per_problem)
        if scenario == "b" and run.cov_scale == 1.0:
            assert 0.0 < shares["rows_at_minus_inf"] < 1.0, shares
            edge = [np.isneginf(res[(q, c)][0][:, -1]) for q, c in res if c % 2]
            assert any(r[0] and not r[-1] for r in edge), "no edge chain stepped inside"
        if scenario in ("a", "f"):
            assert shares["bad"] >= 0.1, shares                                        # at least one proposal in ten at -inf or NaN
        if scenario == "c":
            for (q, c), (rows, st, tr) in res.items():
                if c % 2:
                    assert np.isneginf(rows[:, -1]).all() and (rows[:, :dim] == start[q, c]).all() and st[-1] == 0.0, (q, c)
                    assert np.isneginf(tr[:, 0]).all() and tr[:, 2].all()
                else:
                    assert np.isfinite(rows).all() and st[-1] > 0.0, (q, c)
        if scenario == "d":
            for (q, c), (rows, st, tr) in res.items():
                assert np.isfinite(rows).all() and np.isfinite(st).all() and st[-1] > 0.0, (q, c)
                cov = co.hier_state_covariance(st, dim)
                zero = np.flatnonzero(start[q, c] == 0.0)
                assert len(zero) == (1 if c % 2 else 0)
                for i in zero:                                                         # the zero component never moves, its row of the covariance stays 0
                    assert (rows[:, i] == 0.0).all() and (cov[i] == 0.0).all(), (q, c, i)
                assert (np.delete(np.diag(cov), zero) > 0.0).all(), (q, c)
        if scenario == "e":
            for (q, c), (rows, st, tr) in res.items():
                assert (rows[:, :dim] == start[q, c]).all() and np.isfinite(rows[:, -1]).all() and st[-1] == sc.T, (q, c)
                assert (co.hier_state_covariance(st, dim) == 0.0).all(), (q, c)
        if scenario == "f" and run.cov_scale == 1e8:
            for (q, c), (rows, st, tr) in res.items():
                assert st[-1] == 0.0 and np.isfinite(st).all() and np.isfinite(rows).all(), (q, c)
        if scenario == "g":
            from pyhillfit_amd import hierarchical as H
            shapes, scales, locs = H.prior_params()
            for q, ex in enumerate(exs):
                pk = co.PackedHierPair(ex, shapes, scales, locs)
                assert np.isneginf(pk.ln_conc).sum() == 1 and (pk.ln_conc[np.isfinite(pk.ln_conc)] < -50.0).sum() == 1
                assert sorted(set(pk.response) & {0.0, 100.0, -2.6, 104.0}) == [-2.6, 0.0, 100.0, 104.0]
                assert [len(e) for e in ex] == [len(e) for e in experiments[run.pair[q]]]          # the shape stays
                assert np.isfinite(pk.log_target(run.healthy[q]))
            for (q, c), (rows, st, tr) in res.items():
                assert np.isfinite(rows).all() and st[-1] > 0.0, (q, c)


def test_trace_is_optional_and_changes_nothing(groups):
    """PackedHierPair.advance(trace=True) gives the rows and the state of a plain advance, bit for bit"""
    experiments, theta0 = groups["4 + 4 + 4"]
    run = sc.runs_of("a", theta0, _locs())[0]
    plain, traced = sc.twin_run(run, experiments, chains=[0, 1]), sc.twin_run(run, experiments, chains=[0, 1], trace=True)
    for key in plain:
        for a, b in zip(plain[key], traced[key][:2]):
            assert np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64)), key
