"""The hierarchical kernels at edge states (-m gpu): the hand-allocated gfx950 code object, as plain launches and as the fused persistent
grid, against the hipcc one-lane and two-lane kernels and the scalar twin, bit for bit — chains that sit at -inf (every accept ratio NaN),
starts on and outside every bound of the support, zero-variance directions and a zero covariance (dn = 0 in the factor update, every pivot
non-positive), proposals 1e4 times wider than the start, doses 0 and 1e-30 and responses on and beyond [0, 100] — with healthy and edge
lanes in one wavefront.  The scenario table is tests/hier_edge_scenarios.py; tests/test_hier_edges_host.py holds the twin to the conditions
that keep these comparisons from being vacuous.  A NaN or -inf must be reproduced as a bit pattern, not merely compare equal."""
import numpy as np
import pytest

import hier_edge_scenarios as sc
from test_gpu_isa import _setup
from test_gpu_sl_lean import _same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


HIPCC_ONE_LANE, HIPCC_TWO_LANES, HIPCC_WAVE, ISA, ISA_FUSED = 1, 2, 3, 4, 6          # phf_hierarchical_last_kernel


def _locs():
    from pyhillfit_amd import hierarchical as H
    return H.prior_params()[2]


def _sampler(gpu, oracle_pair, names, experiments, run, lanes, isa, problem_id0=sc.PROBLEM_ID0):
    """the sampler of a run: through test_gpu_isa._setup for Crumb pairs as they are, on the run's own experiments (edited or generated) otherwise"""
    import torch
    from pyhillfit_amd import hierarchical as H
    Q = len(run.pair)
    if names is not None and not run.edited:
        s, _ = _setup(gpu, [names[p] for p in run.pair], oracle_pair, sc.C, sc.THIN, run.adapt, sc.SEED, bool(isa))
    else:
        packed = H.PackedHierPoints(experiments)
        if isa:
            assert (packed.n_expts, packed.points_per_expt) in H.ISA_SHAPES
        s = H.HierarchicalSampler(packed, list(range(Q)), sc.C, thinning=sc.THIN, seed=sc.SEED, adapt_start=run.adapt,
                                  problem_ids=[sc.PROBLEM_ID0 + sc.PROBLEM_ID_STEP * q for q in range(Q)], chain_id_base=sc.CHAIN_ID_BASE, device=gpu)
    if problem_id0 != sc.PROBLEM_ID0:
        s.problem_ids = torch.tensor([problem_id0 + sc.PROBLEM_ID_STEP * q for q in range(Q)], dtype=torch.int32, device=gpu)
        s.prob.problem_id = s.problem_ids.data_ptr()
    s.set_kernel_hint(lanes=lanes, isa=isa)
    s.init(sc.starts(run), cov_scale=run.cov_scale)
    s.enable_moments(after_iteration=sc.MOMENTS_AFTER)
    return s


def _launch(s, cuts=sc.CUTS):
    from pyhillfit_amd import hierarchical as H
    parts, kernels = [], []
    for k in cuts:
        parts.append(s.advance(k).cpu().numpy())
        kernels.append(H.last_kernel())
    Q = s.Q
    return dict(rows=np.concatenate(parts), state=s.state.cpu().numpy().reshape(s.S, Q, sc.C), moments=s.moments.cpu().numpy(), kernels=kernels)


def _launch_fused(samplers, cuts=sc.FUSED_CUTS):
    """the samplers as the groups of ONE persistent grid, quanta of 50 iterations"""
    import torch
    from pyhillfit_amd import hierarchical as H
    f = H.FusedSamplers(samplers)
    f.quantum = 50
    parts, kernels = [], []
    for k in cuts:
        parts.append(f.advance(k))
        kernels.append(H.last_kernel())
    torch.cuda.synchronize()
    f.check_queue()
    return [dict(rows=torch.cat([p[j] for p in parts]).cpu().numpy(), state=s.state.cpu().numpy().reshape(s.S, s.Q, sc.C),
                 moments=s.moments.cpu().numpy(), kernels=kernels) for j, s in enumerate(samplers)]


def _assert_same(a, b, what):
    for name in ("rows", "state", "moments"):
        x, y = np.ascontiguousarray(a[name]).view(np.uint64), np.ascontiguousarray(b[name]).view(np.uint64)
        assert x.shape == y.shape, (what, name)
        same = x == y
        assert same.all(), (what, name, int((~same).sum()), np.argwhere(~same)[:5].tolist())


def _assert_twin(got, run, experiments, what, problem_id0=sc.PROBLEM_ID0):
    """rows and final state — accept count and the factors L diag(d) L' included — of the checked chains"""
    from oracle import c_oracle as co
    dim = run.healthy.shape[1]
    for (q, c), (rows, st) in sc.twin_run(run, experiments, problem_id0=problem_id0).items():
        assert _same_bits(got["rows"][:, q, :, c], rows), (what, "rows", q, c)
        assert _same_bits(got["state"][:, q, c], st), (what, "state", q, c)
        assert _same_bits(co.hier_state_covariance(got["state"][:, q, c], dim), co.hier_state_covariance(st, dim)), (what, "covariance", q, c)


def _assert_scenario(scenario, run, got, what):
    """what the scenario is about did happen, on ALL chains of the launch"""
    from oracle import c_oracle as co
    dim = run.healthy.shape[1]
    rows, state = got["rows"], got["state"]
    assert not np.isnan(rows[:, :, :dim]).any() and np.isfinite(state[:dim]).all(), what
    odd = np.arange(sc.C) % 2 == 1
    if scenario == "c":
        assert (state[-1][:, odd] == 0.0).all() and np.isneginf(rows[:, :, dim][:, :, odd]).all(), what
        assert (state[-1][:, ~odd] > 0.0).all() and np.isfinite(rows[:, :, :, ~odd]).all(), what
    if scenario == "e":
        assert (state[-1] == sc.T).all() and np.isfinite(rows).all(), what
        for q in range(state.shape[1]):
            for c in (0, 63, sc.C - 1):
                assert (co.hier_state_covariance(state[:, q, c], dim) == 0.0).all(), (what, q, c)
    if scenario == "f" and run.cov_scale == 1e8:
        assert (state[-1] == 0.0).all() and np.isfinite(state).all(), what
    if scenario == "b" and run.cov_scale == 1.0:
        share = np.isneginf(rows[:, :, dim][:, :, odd]).mean()
        assert 0.0 < share < 1.0, (what, share)


def _check_run(gpu, oracle_pair, scenario, group, names, experiments, run, isa):
    """hipcc one-lane and two-lane kernel (or, without an assembly kernel, whichever kernel the library picks) and the twin first; the
    assembly only when those agree"""
    what = "%s | %s | %s" % (group, scenario, run.key)
    exs = sc.experiments_of(run, experiments)
    ne = len(exs[0])
    if isa:
        one = _launch(_sampler(gpu, oracle_pair, names, exs, run, 1, False))
        assert one["kernels"] == [HIPCC_ONE_LANE] * len(sc.CUTS), (what, one["kernels"])          # the kernel meant is the kernel that ran
        two = _launch(_sampler(gpu, oracle_pair, names, exs, run, 2, False))
        assert two["kernels"] == [HIPCC_TWO_LANES] * len(sc.CUTS), (what, two["kernels"])
        _assert_same(one, two, what + ": hipcc one lane / two lanes")
    else:
        one = two = _launch(_sampler(gpu, oracle_pair, names, exs, run, 0, None))
        assert one["kernels"] == [HIPCC_ONE_LANE if ne <= 8 else HIPCC_WAVE] * len(sc.CUTS), (what, one["kernels"])
    _assert_twin(one, run, exs, what + ": hipcc / twin")
    _assert_scenario(scenario, run, one, what)
    kernels = {"hipcc": one["kernels"], "hipcc two lanes": two["kernels"]}
    if isa:
        s = _sampler(gpu, oracle_pair, names, exs, run, 1, True)
        asm = _launch(s) if group in sc.PLAIN_ASSEMBLY else _launch_fused([s])[0]
        assert asm["kernels"] == ([ISA] * len(sc.CUTS) if group in sc.PLAIN_ASSEMBLY else [ISA_FUSED] * len(sc.FUSED_CUTS)), (what, asm["kernels"])
        _assert_same(one, asm, what + ": hipcc / assembly")
        _assert_twin(asm, run, exs, what + ": assembly / twin")
        kernels["assembly"] = asm["kernels"]
    print("%s: kernels %s; accepted %.3f, saved rows at -inf %.3f (all %d chains)"
          % (what, kernels, one["state"][-1].mean() / sc.T, np.isneginf(one["rows"][:, :, -1]).mean(), sc.C))


@pytest.mark.parametrize("shape", list(sc.SHAPES))
@pytest.mark.parametrize("scenario", sc.SCENARIOS)
def test_assembly_hipcc_kernels_and_twin_agree_at_edge_states(scenario, shape, gpu, oracle_pair):
    """every run of the scenario on three Crumb pairs of the shape: the hipcc one-lane kernel, the hipcc two-lane kernel and the assembly —
    a plain launch where the code object has a kernel of the shape's own, else a fused grid of this one group (cut on saved rows) —: rows,
    final state with the accept count, moments, bit for bit — and chains {0, 1, 62, 63, 64, 65, C - 2, C - 1} of every problem against
    the twin, final factors included"""
    names, theta0 = sc.SHAPES[shape]
    experiments = [oracle_pair(d, c).experiments for d, c in names]
    for run in sc.runs_of(scenario, theta0, _locs()):
        _check_run(gpu, oracle_pair, scenario, shape, names, experiments, run, True)


@pytest.mark.parametrize("group", list(sc.SYNTHETIC))
@pytest.mark.parametrize("scenario", sc.SYNTHETIC_SCENARIOS)
def test_hipcc_kernels_and_twin_agree_at_edge_states_outside_three_to_six_experiments(scenario, group, gpu, oracle_pair):
    """Ne = 1 and 2 (hier_advance_kernel<1>, <2>, run-time point loops) and Ne = 9 (one wavefront per chain, the per-experiment target
    phf_hier_log_target_by_experiment) on generated pairs, the kernel the library picks, against the twin"""
    experiments, theta0 = sc.synthetic_group(group)
    for run in sc.runs_of(scenario, theta0, _locs()):
        _check_run(gpu, oracle_pair, scenario, group, None, experiments, run, False)


def _fused_runs():
    return [(s, k) for s in sc.FUSED_SCENARIOS for k in range(2 if s == "g" else 1)]


@pytest.mark.parametrize("scenario,which", _fused_runs())
def test_fused_grid_of_fourteen_groups_agrees_with_the_hipcc_launches_at_edge_states(scenario, which, gpu, oracle_pair):
    """the scenario's run on all fourteen launch groups in ONE persistent grid (quanta of 50 iterations; launches before, across and after
    adapt_start, each starting on a saved row): rows, state and moments of every group against its own hipcc launches, which are held to the
    twin first; the queue's fault word stays clear"""
    runs, exss, want = [], [], []
    for j, (names, theta0) in enumerate(sc.FOURTEEN):
        run = sc.runs_of(scenario, theta0, _locs())[which]
        exs = sc.experiments_of(run, [oracle_pair(d, c).experiments for d, c in names])
        ref = _launch(_sampler(gpu, oracle_pair, names, exs, run, 1, False, problem_id0=100 * j + sc.PROBLEM_ID0), sc.FUSED_CUTS)
        assert ref["kernels"] == [HIPCC_ONE_LANE] * len(sc.FUSED_CUTS), (j, ref["kernels"])
        _assert_twin(ref, run, exs, "group %d | %s | %s: hipcc / twin" % (j, scenario, run.key), problem_id0=100 * j + sc.PROBLEM_ID0)
        runs.append(run); exss.append(exs); want.append(ref)
    fus = [_sampler(gpu, oracle_pair, names, exs, run, 1, True, problem_id0=100 * j + sc.PROBLEM_ID0)
           for j, ((names, _), run, exs) in enumerate(zip(sc.FOURTEEN, runs, exss))]
    got = _launch_fused(fus)
    for j, (g, ref) in enumerate(zip(got, want)):
        assert g["kernels"] == [ISA_FUSED] * len(sc.FUSED_CUTS), (j, g["kernels"])
        _assert_same(ref, g, "group %d | %s | %s: hipcc / fused grid" % (j, scenario, runs[j].key))
    print("fused | %s | %s: kernel %d on fourteen groups" % (scenario, runs[0].key, ISA_FUSED))
