"""Power-scaling sensitivity on the GPU (phf_sensitivity_*): the device's components equal the host build of phf_sensitivity.h bit for
bit; counts, masses and counters equal the numpy restatement of test_sensitivity_host.py integer for integer and the per-chain sums the
host header's accumulation bit for bit, however the rows are cut; the conjugate-normal known answer through the device path; and the
command lines' --sensitivity against chain_sensitivity on the files they wrote."""
import functools
import json

import numpy as np
import pytest

from test_gpu_waic import _summaries, csv_file, dr_setup, gpu  # noqa: F401
from test_sensitivity_host import (Restatement, build_shim, conjugate_normal, host_chain_sums, host_cjs_sums, host_hier_components,
                                   host_sl_components, host_weights)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("sensitivity_gpu"))


def synthetic_pairs():
    """two single-level pairs with entries censored at 0 and at 100, replicates to merge, and an odd number of entries"""
    from pyhillfit_amd import doseresponse as dr
    c1 = np.array([0.01, 0.1, 1.0, 10.0, 100.0] * 3)
    y1 = np.array([0.0, 4.0, 31.0, 77.0, 100.0, 0.0, 6.5, 28.0, 81.0, 100.0, 1.5, 0.0, 35.0, 74.0, 97.0])
    c2 = np.array([0.3, 3.0, 30.0, 300.0, 0.3, 3.0, 30.0])
    y2 = np.array([2.0, 22.0, 64.0, 100.0, 0.0, 18.0, 70.0])
    return dr.PackedPoints([(c1, y1), (c2, y2)])


def synthetic_experiments(ne, rng):
    out = []
    for e in range(ne):
        n = 4 if e % 3 else 5
        conc = np.array([0.03, 0.3, 3.0, 30.0, 300.0])[:n]
        y = np.clip(100.0 / (1.0 + (1.0 / conc) ** 0.9) + rng.normal(0.0, 4.0, n), 0.5, 99.5)
        out.append(np.column_stack([conc, y]))
    return out


def _special(theta, rng, support_rows):
    """overwrite the first rows of theta [m][d] with out-of-support, NaN and infinite entries"""
    k = 0
    for row in support_rows:
        theta[k] = row; k += 1
    d = theta.shape[1]
    for v in (np.nan, np.inf, -np.inf):
        for j in range(d):
            theta[k, j] = v; k += 1
    theta[k] = np.nan
    return theta


@pytest.mark.parametrize("model", [1, 2])
def test_single_level_components_equal_the_host_build(gpu, shim, model):
    from pyhillfit_amd import sensitivity as sn
    from pyhillfit_amd.sampler import DevicePoints
    packed = synthetic_pairs()
    rng = np.random.default_rng(model)
    m, d = 200, model + 1
    theta = np.column_stack([rng.normal(5.5, 1.5, m), rng.uniform(0.1, 3.0, m), np.exp(rng.normal(1.5, 1.0, m))])
    theta = theta if model == 2 else theta[:, [0, 2]]
    edge = [[-3.5, 1.0, 5.0], [-3.0, 1.0, 5.0], [5.0, -0.1, 5.0], [5.0, 10.5, 5.0], [5.0, 1.0, 1e-3], [5.0, 1.0, 5e-4], [5.0, 0.0, 5.0], [40.0, 9.0, 0.01]]
    theta = _special(theta, rng, [e if model == 2 else [e[0], e[2]] for e in edge])
    pidx = (np.arange(m) % 2).astype(np.int32)
    got = sn.components(DevicePoints(packed, gpu), model, pidx, theta, device=gpu)
    for q in range(2):
        sel = pidx == q
        want = host_sl_components(shim, packed, q, model, theta[sel])
        assert np.array_equal(got[0, sel], want[0], equal_nan=True) and np.array_equal(got[1, sel], want[1], equal_nan=True), q
        assert np.all(got[2, sel] == 0.0)
    assert np.isneginf(got[0]).sum() >= 3 and np.isfinite(got[:2]).all(axis=0).sum() > 150


@pytest.mark.parametrize("ne", [1, 3, 9])
def test_hierarchical_components_equal_the_host_build(gpu, shim, ne):
    from pyhillfit_amd import hierarchical as H
    from pyhillfit_amd import sensitivity as sn
    rng = np.random.default_rng(10 + ne)
    packed = H.PackedHierPoints([synthetic_experiments(ne, rng), synthetic_experiments(ne, rng)])
    prior = H.make_prior()
    m, dim = 200, 5 + 2 * ne
    theta = np.column_stack([rng.uniform(0.3, 3.0, m), rng.uniform(2.1, 9.0, m), rng.uniform(3.0, 8.0, m), rng.uniform(0.05, 1.5, m)]
                            + [f(m) for _ in range(ne) for f in (lambda k: rng.uniform(3.0, 8.0, k), lambda k: np.exp(rng.uniform(-1.0, 1.0, k)))]
                            + [np.exp(rng.uniform(np.log(0.3), np.log(40.0), m))])
    good = theta[0].copy()
    edge = []
    for j, v in ((0, 0.0), (1, 2.0), (2, -4.0), (3, 0.01), (dim - 1, 1e-3), (4, -2.5), (5, -0.5), (5, 1e-300), (4, 400.0)):
        e = good.copy(); e[j] = v; edge.append(e)
    theta = _special(theta, rng, edge)
    pidx = (np.arange(m) % 2).astype(np.int32)
    got = sn.components(H.DeviceHierPoints(packed, gpu), "hierarchical", pidx, theta, prior=prior, device=gpu)
    for q in range(2):
        sel = pidx == q
        want = host_hier_components(shim, packed, q, prior, theta[sel])
        for k in range(3):
            assert np.array_equal(got[k, sel], want[k], equal_nan=True), (q, k)
    assert np.isneginf(got[0]).sum() >= 5 and np.isfinite(got).all(axis=0).sum() > 100


# ---- the accumulation -----------------------------------------------------------------------------------------------------------
ROWS, CHAINS, DELTA, BINS = 37, 65, 0.25, 256


@functools.lru_cache(maxsize=None)
def structured_rows():
    """[37][2][4][65] model-2 rows (the fourth column is never read): 2 problems x 65 chains (a full wavefront and a tail lane) x 37
    rows; one NaN row; one chain whose prior component is -inf throughout; one problem whose first draw is not finite"""
    rng = np.random.default_rng(7)
    x = np.empty((ROWS, 2, 4, CHAINS))
    x[:, :, 0] = rng.normal(0.0, 0.12, (ROWS, 2, CHAINS)) + np.array([5.75, 4.9])[None, :, None]
    x[:, :, 1] = np.exp(rng.normal(-0.4, 0.12, (ROWS, 2, CHAINS)))
    x[:, :, 2] = np.exp(rng.normal(2.0, 0.3, (ROWS, 2, CHAINS)))
    x[:, :, 3] = np.nan
    x[5, 0, :3, :] = np.nan                                     # a NaN row of problem 0
    x[:, 0, 0, 7] = -3.5                                        # chain 7 of problem 0: pIC50 below the prior's support throughout
    x[0, 1, :3, 0] = np.nan                                     # problem 1's first draw
    x[3, 1, 2, 11] = np.inf                                     # one infinite sigma
    return x


def feed(x, cuts, kind, points, device, delta=DELTA, bins=BINS, cols=3, given=None, prior=None):
    from pyhillfit_amd.sensitivity import PowerScaling
    ps = PowerScaling(points, kind, x.shape[1], x.shape[3], cols, x.shape[0], delta, bins, device, given=given, prior=prior)
    t = torch.from_numpy(x).to(device)
    r0 = 0
    for n in cuts:
        ps.accumulate(t[r0:r0 + n].contiguous())
        r0 += n
    assert r0 == x.shape[0]
    return ps


def restate(shim, x, comps, delta, bins):
    am1 = (shim.v_alpha_m1(delta, 0), shim.v_alpha_m1(delta, 1))
    return Restatement(x, comps, delta, bins, functools.partial(host_weights, shim), alpha_m1=am1)


def check_against_restatement(ps, shim, x, comps_of, cols):
    """ps fed x [n][Q][stride][C]; comps_of(q) -> [2][n][C], the host's components of problem q"""
    counts = ps.counts()
    slots, weights, colsums, pc_w, pc_c = ps.reduced(per_chain=True)
    n, Q, _, Cn = x.shape
    seen_clamped = 0
    for q in range(Q):
        xq = np.ascontiguousarray(x[:, q, :cols, :])
        r = restate(shim, xq, comps_of(q), ps.delta, ps.B)
        assert np.array_equal(counts[q], r.counts), q
        for s in range(4):
            entered = n * Cn - r.non_finite[s // 2]
            assert weights[q, s, 0] == entered and weights[q, s, 3] == r.clamped[s], (q, s)
        seen_clamped += int(r.clamped.sum())
        for j in range(cols):
            assert slots[q, j, 3] == r.nonfinite_values[j] and slots[q, j, 2] == r.counts[j, 0].sum()
            assert slots[q, j, 5] == r.level[j] and slots[q, j, 6] == r.anchor[j] and slots[q, j, 7] == r.w0[j]
            v = xq[:, j, :][np.isfinite(xq[:, j, :])]
            assert slots[q, j, 0] == v.min() and slots[q, j, 1] == v.max()
            for s in range(4):                                  # the device's CJS sums are the host header's on the same integers
                assert np.array_equal(slots[q, j, 8 + 5 * s:13 + 5 * s], host_cjs_sums(shim, r.counts[j, 0], r.counts[j, 1 + s])), (q, j, s)
        wsum, csum = host_chain_sums(shim, r, xq)
        assert np.array_equal(pc_w[q], wsum), q                 # bit for bit
        assert np.array_equal(pc_c[q], csum), q
        # the merged sums: the chains in chain order
        merged = np.zeros_like(wsum[..., 0])
        for c in range(Cn):
            merged += wsum[..., c]
        assert np.array_equal(weights[q], merged)
    return seen_clamped


def test_counts_masses_and_sums_equal_the_restatement(gpu, shim):
    from pyhillfit_amd.sampler import DevicePoints
    x, packed = structured_rows(), synthetic_pairs()
    ps = feed(x, (ROWS,), 2, DevicePoints(packed, gpu), gpu)

    def comps_of(q):
        th = x[:, q, :3, :].transpose(0, 2, 1).reshape(-1, 3)
        return host_sl_components(shim, packed, q, 2, th)[:2].reshape(2, ROWS, CHAINS)

    c0 = comps_of(0)
    others = [r for r in range(ROWS) if r != 5]                 # (row 5 is the NaN row)
    assert np.isneginf(c0[0, others, 7]).all() and np.isfinite(c0[1, others, 7]).all()   # the -inf chain: the prior only
    assert not np.isfinite(comps_of(1)[:, 0, 0]).any()          # problem 1's first draw: c_ref is a later one
    clamped = check_against_restatement(ps, shim, x, comps_of, 3)
    assert clamped > 0                                          # delta = 0.25: some draws clamp
    res = ps.result()
    assert res["non_finite"][0, 0] == CHAINS + (ROWS - 1) and res["non_finite"][0, 1] == CHAINS   # the NaN row; and, prior, chain 7
    for q in range(2):
        assert list(res["non_finite"][q]) == [int((~np.isfinite(c)).sum()) for c in comps_of(q)]
    assert res["non_finite"][1].min() >= 1
    assert np.all(res["ess_fraction"] > 0) and np.all(res["ess_fraction"] <= 1.0)


@pytest.mark.parametrize("cuts", [(1, 36), (5, 17, 15), (36, 1)])
def test_cuts_are_bit_identical(gpu, cuts):
    from pyhillfit_amd.sampler import DevicePoints
    x, pts = structured_rows(), DevicePoints(synthetic_pairs(), gpu)
    whole, part = feed(x, (ROWS,), 2, pts, gpu), feed(x, cuts, 2, pts, gpu)
    assert np.array_equal(whole.counts(), part.counts())
    for a, b in zip(whole.reduced(per_chain=True), part.reduced(per_chain=True)):
        assert np.array_equal(a, b, equal_nan=True)


def test_level_change_between_calls(gpu, shim):
    """kind "given": the second call's values range 1 000 times as far as the first's, so every slot's grid coarsens between the
    calls and the five arrays merge"""
    rng = np.random.default_rng(11)
    n, Cn = 24, 65
    x = np.empty((n, 1, 4, Cn))
    x[:, 0, 0] = rng.normal(2.0, 1.0, (n, Cn)); x[:, 0, 1] = rng.normal(-1.0, 0.01, (n, Cn))
    x[12:, 0, :2] = (x[12:, 0, :2] - [[2.0], [-1.0]]) * 1000.0 + [[2.0], [-1.0]]
    x[:, 0, 2] = rng.normal(0.0, 16.0, (n, Cn)); x[:, 0, 3] = rng.normal(-40.0, 6.0, (n, Cn))
    first = feed(x[:12], (12,), "given", None, gpu, cols=2, given=(2, 3))
    ps = feed(x, (12, 12), "given", None, gpu, cols=2, given=(2, 3))
    comps = np.stack([x[:, 0, 2], x[:, 0, 3]])
    assert check_against_restatement(ps, shim, x, lambda q: comps, 2) > 0
    assert np.all(ps.reduced()[0][0, :, 5] >= first.reduced()[0][0, :, 5] + 9)     # 1 000 x the range: about ten levels up


def test_known_answer_through_the_device(gpu, shim):
    from pyhillfit_amd import sensitivity as sn
    rows, delta = conjugate_normal(), 0.01
    x = np.ascontiguousarray(rows[:, None])                     # [4000][1][3][64]: theta, then the two components
    ps = feed(x, (1500, 2500), "given", None, gpu, delta=delta, bins=4096, cols=1, given=(1, 2))
    res = ps.result()
    r = restate(shim, rows[:, :1], rows[:, 1:].transpose(1, 0, 2), delta, 4096)
    assert np.array_equal(ps.counts()[0], r.counts)
    for comp in range(2):
        sums = [host_cjs_sums(shim, r.counts[0, 0], r.counts[0, 1 + 2 * comp + d]) for d in range(2)]
        cjs = [float(sn.cjs_from_sums(*s[:4])) for s in sums]
        want = float(sn.sensitivity_d(cjs[0], cjs[1], delta))
        assert res["D"][0, 0, comp] == want                      # the host restatement's D, exactly
        numpy_d = r.D(0, comp, sn.cjs_numpy) / (2.0 * np.log2(1.0 + delta))
        assert want == pytest.approx(numpy_d, rel=1e-9)
    assert res["D"][0, 0, 0] == pytest.approx(0.0235, abs=0.002) and res["D"][0, 0, 1] == pytest.approx(0.085, abs=0.006)
    assert res["diagnosis"][0, 0] == "likelihood-dominated"
    theta = rows[:, 0]
    assert res["base_mean"][0, 0] == pytest.approx(theta.mean(), rel=1e-12) and res["base_sd"][0, 0] == pytest.approx(theta.std(), rel=1e-10)
    for comp in range(2):
        for d in range(2):
            w = r.w[2 * comp + d]
            mw = (w * theta).sum() / w.sum()
            assert res["mean_shift"][0, 0, comp, d] == pytest.approx((mw - theta.mean()) / theta.std(), rel=1e-8)
            per_chain = (w * theta).sum(axis=0) / w.sum(axis=0) - theta.mean(axis=0)
            assert res["mean_shift_se"][0, 0, comp, d] == pytest.approx(per_chain.std(ddof=1) / 8.0 / theta.std(), rel=1e-8)
            assert res["ess_fraction"][0, comp, d] == pytest.approx(w.sum() ** 2 / (w.size * (w * w).sum()), rel=1e-12)
    assert np.all(res["clamped"] == 0) and np.all(res["non_finite"] == 0)


# ---- one grid, two users ----------------------------------------------------------------------------------------------------------
GRID_ROWS, GRID_CUTS = 36, ((36,), (5, 17, 14))


def grid_rows(Cn):
    """[36][2][5][Cn]: three parameter columns — a constant, a normal with NaN and +-inf sprinkled in, one whose range grows 2^20-fold
    from row 5 on (the second cut of (5, 17, 14)) — and two finite columns, the given components"""
    rng = np.random.default_rng(100 + Cn)
    x = np.empty((GRID_ROWS, 2, 5, Cn))
    x[:, :, 0] = np.array([7.25, -0.003])[None, :, None]
    x[:, :, 1] = rng.normal(-2.0, 0.7, (GRID_ROWS, 2, Cn))
    x[0, 1, 1, 0] = np.nan                                      # problem 1's first value: a later one anchors the grid
    x[2, 0, 1, 1], x[5, 0, 1, Cn - 1], x[20, 1, 1, 3], x[35, 0, 1, 0] = np.inf, -np.inf, np.nan, np.inf
    x[:, :, 2] = 3.0 + rng.normal(0.0, 1e-4, (GRID_ROWS, 2, Cn))
    x[5:, :, 2] = (x[5:, :, 2] - 3.0) * 2.0 ** 20 + 3.0
    x[:, :, 3] = rng.normal(0.0, 16.0, (GRID_ROWS, 2, Cn)); x[:, :, 4] = rng.normal(-40.0, 6.0, (GRID_ROWS, 2, Cn))
    return x


def grid_state(obj, arrays):
    """(base counts [Q][cols][B], header [Q][cols][8] as bit patterns, non-finite counts [Q][cols]) of a workspace that starts with
    [slots][arrays][B] uint64 counts, [slots][8] header doubles and [slots] uint64 non-finite counts"""
    S = obj.Q * obj.cols
    raw = obj.ws.view(torch.int64).cpu().numpy().view(np.uint64)
    n = S * arrays * obj.B
    return (raw[:n].reshape(obj.Q, obj.cols, arrays, obj.B)[:, :, 0], raw[n:n + 8 * S].reshape(obj.Q, obj.cols, 8),
            raw[n + 8 * S:n + 9 * S].reshape(obj.Q, obj.cols))


@pytest.mark.parametrize("bins", [64, 4096])
@pytest.mark.parametrize("Cn", [5, 96])
def test_quantiles_and_sensitivity_share_one_grid(gpu, Cn, bins):
    """the same rows through phf_quantiles_accumulate and through phf_sensitivity_accumulate (kind "given"): per slot the base counts,
    the eight header doubles and the non-finite count are equal as integers and bit patterns, and the same however the rows are cut"""
    from pyhillfit_amd.quantiles import PosteriorQuantiles
    x = grid_rows(Cn)
    t = torch.from_numpy(x).to(gpu)
    states = []
    for cuts in GRID_CUTS:
        qn = PosteriorQuantiles(2, Cn, 3, GRID_ROWS, bins=bins, device=gpu)
        r0 = 0
        for n in cuts:
            qn.accumulate(t[r0:r0 + n].contiguous())
            r0 += n
        ps = feed(x, cuts, "given", None, gpu, bins=bins, cols=3, given=(3, 4))
        q_counts, q_nf = qn.counts()
        q_state, s_state = grid_state(qn, 1), grid_state(ps, 5)
        assert np.array_equal(q_state[0], q_counts) and np.array_equal(q_state[2], q_nf)     # the accessors read the same words
        assert np.array_equal(s_state[0], ps.counts()[:, :, 0])
        for got, want in zip(s_state, q_state):
            assert got.dtype == np.uint64 and np.array_equal(got, want), cuts
        states.append(q_state)
    for a, b in zip(*states):
        assert np.array_equal(a, b)
    counts, hdr, nf = states[0]
    level = hdr.view(np.float64)[:, :, 4]
    assert np.all(counts.sum(axis=2) + nf == GRID_ROWS * Cn) and list(nf[:, 1]) == [3, 2] and np.all(nf[:, [0, 2]] == 0)
    assert np.all((counts[:, 0] != 0).sum(axis=1) == 1) and np.all(level[:, 0] == 0)          # the constant: one bin, level 0
    # the third column's level after the first cut alone: the second cut raises it by more than log2 B, the merge's D clamp
    first = PosteriorQuantiles(2, Cn, 3, GRID_ROWS, bins=bins, device=gpu)
    first.accumulate(t[:5].contiguous())
    level5 = grid_state(first, 1)[1].view(np.float64)[:, :, 4]
    assert np.all(level[:, 2] > level5[:, 2] + np.log2(bins))


# ---- command lines --------------------------------------------------------------------------------------------------------------
def _strip(s):
    s.pop("mh_samples_per_second")
    return s


def test_single_level_cli(csv_file, tmp_path):  # noqa: F811
    from pyhillfit_amd import PyHillFit
    from pyhillfit_amd.chain_sensitivity import sensitivity_file
    base = ["--data-file", csv_file, "-m", "2", "-i", "5000", "--drugs", "Amiodarone,Bepridil", "--channels", "hERG", "--num-chains", "64",
            "--segment", "2000", "--save-all-chains"]
    PyHillFit.main(base + ["--output-root", str(tmp_path / "on"), "--sensitivity"])
    PyHillFit.main(base + ["--output-root", str(tmp_path / "off")])
    on, off = _summaries(str(tmp_path / "on")), _summaries(str(tmp_path / "off"))
    assert len(on) == 2 and len(off) == 2
    for (path, s_on), s_off in zip(on.items(), off.values()):
        assert "sensitivity" not in s_off
        rec = s_on.pop("sensitivity")
        assert _strip(s_on) == _strip(s_off)
        assert list(rec["columns"]) == ["pIC50", "Hill", "sigma"] and rec["delta"] == 0.01 and rec["bins"] == 4096
        tool = sensitivity_file(path.replace("_summary.json", "_all_chains.npy"))
        assert {k: tool[k] for k in rec} == json.loads(json.dumps(rec))
        assert tool["chains"] == 64 and rec["columns"]["pIC50"]["draws"] == 64 * s_off["saved_rows_after_burn_in"]
        for comp in ("prior", "likelihood"):
            assert rec["weights"][comp]["non_finite"] == 0 and min(rec["weights"][comp]["ess_fraction"]) > 0.5
            for col in rec["columns"].values():
                assert col[comp]["D"] is not None and col[comp]["D"] >= 0.0


def test_hierarchical_cli(csv_file, dr_setup, tmp_path):  # noqa: F811
    from pyhillfit_amd import PyHillFit
    from pyhillfit_amd.chain_sensitivity import main as tool_main
    dr = dr_setup
    pick = None
    for ch in dr.channels:                                       # one channel with a 3-experiment and a 4-experiment pair
        by_ne = {}
        for d in dr.drugs:
            try:
                by_ne.setdefault(dr.load_crumb_data(d, ch)[0], d)
            except Exception:
                continue
        if 3 in by_ne and 4 in by_ne:
            pick = (by_ne[3], by_ne[4], ch)
            break
    assert pick is not None
    base = ["--data-file", csv_file, "-m", "2", "--hierarchical", "-i", "4000", "--drugs", pick[0] + "," + pick[1], "--channels", pick[2],
            "--num-chains", "1", "--segment", "1500"]
    PyHillFit.main(base + ["--output-root", str(tmp_path / "on"), "--sensitivity", "--sensitivity-delta", "0.05"])
    PyHillFit.main(base + ["--output-root", str(tmp_path / "off")])
    on, off = _summaries(str(tmp_path / "on")), _summaries(str(tmp_path / "off"))
    assert sorted(s["num_expts"] for s in on.values()) == [3, 4] and len(off) == 2
    for (path, s_on), s_off in zip(on.items(), off.values()):
        assert "sensitivity" not in s_off
        rec = s_on.pop("sensitivity")
        assert _strip(s_on) == _strip(s_off)
        ne = s_on["num_expts"]
        assert len(rec["columns"]) == 5 + 2 * ne and list(rec["columns"])[:4] == ["alpha", "beta", "mu", "s"] and rec["delta"] == 0.05
        # the chain file holds the run's one chain: the tool on it gives the record exactly
        import contextlib
        import io
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            tool_main(["--data-file", csv_file, "--hierarchical", "--delta", "0.05", path.replace("_summary.json", ".txt")])
        tool = json.loads(out.getvalue())
        assert tool["model"] == "hierarchical" and tool["chains"] == 1
        assert {k: tool[k] for k in rec} == json.loads(json.dumps(rec))
        assert all(rec["columns"][n]["prior"]["D"] is not None for n in rec["columns"])
