"""The ten pnp_* kernels of csrc/visloc.hip through the C ABI (d3r_pnp_ransac) against restated_pnp_ransac of tests/test_visloc_cpu.py, round
by round, and d3r_match_pairs at its 1024 tile.

What is compared how:
  * (status, drawn, best_h): EXACTLY. They are integers decided by supports, and test_every_gpu_case_is_unambiguous (CPU) has asserted for
    every case here that no point within the band thr (1 +- 1e-3) decides a round; the band and its width are derived in
    restated_pnp_ransac's docstring (FMA contraction and the device's libm move the kernel's fp32 test by < 1.5e-4 px).
  * the mask and out_inliers: the mask is 0 / 1, its sum is out_inliers, and it equals the fp64 gate (test_visloc_cpu.gate_sets) at the
    RETURNED pose. The CPU cannot know the polished pose in advance, so where a point lies inside the band at that pose the job asserts
    lo <= mask <= hi instead; the share of such jobs in the round matrix must stay below 5 %.
  * poses: noiseless problems to the 1e-6 of test_pnp_synthetic; the polish on noisy data to 1e-5 against the fp64 _lm_reference started
    from the restated best pose over the restated best set (both sit at the same minimiser).
  * a job alone against the same job in a batch: pose bytes, mask and stats bit for bit.
No speed is asserted anywhere."""
import numpy as np
import pytest
import torch

from test_visloc_cpu import (BIG_SEED, CHUNK, K, MANY_JOBS, RND, ROUND_NS, _case, budget_cases, cheirality_cases, gate_sets, lm_case, many_jobs,
                             non_finite_cases, pnp_abi, pnp_problem, restated, round_cases, seed_cases)
from test_visloc_gpu import _expected_matches, _lm_reference

pytestmark = pytest.mark.gpu


def _same_rounds(case, got, max_points=None):
    want = restated(case, max_points)
    assert want['unambiguous'], case['name']
    assert (got[0], got[2], got[3]) == (want['status'], want['drawn'], want['best_h']), (case['name'], got, want['best_support'])
    return want


def _mask_at_the_returned_pose(case, got, pose, mask):
    """the mask against the fp64 gate at the pose that came back; True when a point inside the band made it a comparison by inclusion"""
    assert set(np.unique(mask).tolist()) <= {0, 1} and got[1] == int(mask.sum()), case['name']
    if not got[0]:
        assert not mask.any() and not pose.any(), case['name']
        return False
    lo, hi = gate_sets(pose, case['uv'], case['X'], case['thr'])
    m = mask.astype(bool)
    if np.array_equal(lo, hi):
        assert np.array_equal(m, lo), (case['name'], np.flatnonzero(m != lo))
        return False
    assert (lo <= m).all() and (m <= hi).all(), case['name']
    return True


def _bit_equal(a, b, k):
    (sa, pa, ma), (sb, pb, mb) = a, b
    assert sa == sb and pa.tobytes() == pb.tobytes() and ma.tobytes() == mb.tobytes(), k


def _batch_and_alone(cases, gpu):
    """the cases as one call and each as a call of its own (the same bits): [(stats, pose, mask)] of the batch"""
    batch = list(zip(*pnp_abi(cases, gpu, params=(max(c['max_iters'] for c in cases), max(len(c['uv']) for c in cases)))))
    for k, case in enumerate(cases):
        alone = pnp_abi([case], gpu)
        _bit_equal(batch[k], (alone[0][0], alone[1][0], alone[2][0]), case['name'])
    return batch


def _pose_err(pose, w2c):
    return np.abs(pose - w2c[:3]).max()


# ---- a. round by round -----------------------------------------------------------------------------------------------------------------------
_BY_INCLUSION = {}


def _round_matrix(gpu, n):
    cases = round_cases(n)
    by_inclusion = 0
    for case, (got, pose, mask) in zip(cases, _batch_and_alone(cases, gpu)):
        _same_rounds(case, got)
        by_inclusion += _mask_at_the_returned_pose(case, got, pose, mask)
    _BY_INCLUSION[n] = (by_inclusion, len(cases))


@pytest.mark.parametrize('n', ROUND_NS)
def test_rounds_equal_the_restatement(gpu, n):
    _round_matrix(gpu, n)


def test_share_of_jobs_compared_by_inclusion(gpu):
    for n in ROUND_NS:
        if n not in _BY_INCLUSION:                                 # run on its own
            _round_matrix(gpu, n)
    by_inclusion, jobs = (sum(v[k] for v in _BY_INCLUSION.values()) for k in (0, 1))
    print(f'round matrix: {by_inclusion} of {jobs} jobs compared by inclusion', {n: v[0] for n, v in _BY_INCLUSION.items()})
    assert jobs == 216 and by_inclusion < 0.05 * jobs


# ---- b. budgets ------------------------------------------------------------------------------------------------------------------------------
def test_budgets_that_are_no_multiple_of_a_round(gpu):
    cases = budget_cases()
    batch = _batch_and_alone(cases, gpu)
    for case, (got, pose, mask) in zip(cases, batch):
        want = _same_rounds(case, got)
        assert want['drawn'] == case['max_iters'] or want['drawn'] % RND == 0
        _mask_at_the_returned_pose(case, got, pose, mask)
    assert [b[0][2] for b in batch[:4]] == [1, 127, 128, 129]
    # the job's own budget of 129 inside a call that launches 1024 / 128 rounds: the same job, bit for bit
    stats, poses, masks = pnp_abi([cases[3]], gpu, params=(1024, 300))
    _bit_equal((stats[0], poses[0], masks[0]), batch[3], 'budget 129 of 1024')


def test_jobs_that_do_not_run(gpu):
    runs = budget_cases()[4]
    none = _case('max_iters 0', runs['uv'], runs['X'], max_iters=0)
    uv, X, _, _ = pnp_problem(1500, 0.0, 0.0, 9)
    big = _case('n above max_points', uv, X, max_iters=300)
    stats, poses, masks = pnp_abi([none, big, runs], gpu, params=(300, 1000))
    assert stats[0] == (0, 0, 0, -1) and not masks[0].any() and not poses[0].any()
    # the count kernel's grid is sized by max_points: one workgroup of CHUNK rows, which it clears; the rows behind stay as they were
    assert stats[1] == (0, 0, 0, -1) and not masks[1][:CHUNK].any() and (masks[1][CHUNK:] == 7).all() and not poses[1].any()
    for case, k in ((none, 0), (big, 1), (runs, 2)):
        _same_rounds(case, stats[k], max_points=1000)
    assert stats[2][0] == 1
    _bit_equal((stats[2], poses[2], masks[2]), [x[0] for x in pnp_abi([runs], gpu)], 'beside jobs that do not run')


# ---- c. cheirality ---------------------------------------------------------------------------------------------------------------------------
def test_points_behind_the_camera_are_no_inliers(gpu):
    cases = cheirality_cases()
    for case, (got, pose, mask) in zip(cases, _batch_and_alone(cases, gpu)):
        want = _same_rounds(case, got)
        kept = ~case['mirrored']
        assert got[0] == 1 and got[1] == kept.sum() == {600: 400, 1025: 683}[len(kept)] and want['drawn'] == RND
        assert np.array_equal(mask.astype(bool), kept)
        assert _pose_err(pose, case['w2c']) < 1e-6


# ---- d. non-finite rows ----------------------------------------------------------------------------------------------------------------------
def test_non_finite_rows_are_no_inliers_and_do_not_freeze_the_polish(gpu):
    cases = non_finite_cases()
    batch = list(zip(*pnp_abi(cases, gpu)))
    for case, (got, pose, mask) in zip(cases, batch):
        print(case['name'], got, 'spoilt rows in the mask:', np.flatnonzero(mask.astype(bool) & case['spoilt']).tolist(),
              'pose error', _pose_err(pose, case['w2c']))
    for case, (got, pose, mask) in zip(cases, batch):
        _bit_equal((got, pose, mask), [x[0] for x in pnp_abi([case], gpu)], case['name'])
        _same_rounds(case, got)
        assert got[0] == 1 and got[1] == (~case['spoilt']).sum() and np.array_equal(mask.astype(bool), ~case['spoilt']), case['name']
        # the polished pose: a NaN in the first LM sums would leave the best hypothesis as it was solved, which need not be this close
        assert _pose_err(pose, case['w2c']) < 1e-6, case['name']


# ---- e. more than 64 jobs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_jobs', MANY_JOBS)
def test_more_jobs_than_a_workgroup_of_the_per_job_kernels(gpu, n_jobs):
    cases = many_jobs(n_jobs)
    batch = _batch_and_alone(cases, gpu)
    for case, (got, pose, mask) in zip(cases, batch):
        _same_rounds(case, got)
        _mask_at_the_returned_pose(case, got, pose, mask)
        assert not (case.get('fails') and got[0])
    failing = [k for k, c in enumerate(cases) if c.get('fails')]
    assert failing == sorted({0, 63, 64, n_jobs - 1} & set(range(n_jobs))) and sum(b[0][0] for b in batch) > n_jobs // 2
    assert batch[0][0] == (0, 0, 0, -1) and batch[63][0][2] == 300


# ---- f. the LM set ---------------------------------------------------------------------------------------------------------------------------
def test_the_polish_runs_over_the_best_hypothesis_inliers_as_scored(gpu):
    case = lm_case()
    want = restated(case)
    assert want['lo'].sum() < case['planted'].sum() and (want['lo'] <= case['planted']).all()       # a strict subset of the planted set
    (got,), (pose,), (mask,) = pnp_abi([case], gpu)
    _same_rounds(case, got)
    start = np.eye(4)
    start[:3] = want['pose']
    ref = _lm_reference(case['uv'][want['lo']], case['X'][want['lo']], start)
    over_planted = _lm_reference(case['uv'][case['planted']], case['X'][case['planted']], start)
    print('LM over the best set: largest deviation from the fp64 reference', _pose_err(pose, ref), '; the planted set\'s minimiser is',
          _pose_err(over_planted[:3], ref), 'away')
    assert _pose_err(pose, ref) < 1e-5
    _mask_at_the_returned_pose(case, got, pose, mask)


# ---- 3. the matching kernels at their tile, the seed's width -----------------------------------------------------------------------------------
def test_match_pairs_at_the_tile_edges(gpu):
    """one pair per combination of 1023, 1024 and 1025 compacted points on the two sides (match_compact's and match_mutual's 1024 threads,
    match_nn's 1024 queries per workgroup and 1024 points per LDS tile), the confidences planted so that the counts are exact"""
    from dust3r_amd.visloc import match_pairs
    g = torch.Generator(device='cpu').manual_seed(17)
    H, W, thr = 32, 40, 1.5
    pairs, counts = [], []
    for nq in (1023, 1024, 1025):
        for nm in (1023, 1024, 1025):
            pq = torch.randn((H, W, 3), generator=g)
            pm = pq + 0.01 * torch.randn((H, W, 3), generator=g) if (nq + nm) % 2 else torch.randn((H, W, 3), generator=g)
            cq, cm = torch.full((H * W,), 1.0), torch.full((H * W,), 1.0)
            cq[torch.randperm(H * W, generator=g)[:nq]] = 2.0
            order = torch.randperm(H * W, generator=g)
            cm[order[:nm]] = 1.5                                          # at the threshold: used
            vm = torch.ones(H * W, dtype=torch.bool)
            cm[order[nm:nm + 100]] = 3.0                                  # confident but invalid: not used
            vm[order[nm:nm + 100]] = False
            pairs.append((pq, cq.reshape(H, W), pm, cm.reshape(H, W), vm.reshape(H, W)))
            counts.append((nq, nm))
    got = match_pairs([tuple(t.to(gpu) for t in p) for p in pairs], thr, gpu)
    total = 0
    for (pq, cq, pm, cm, vm), (nq, nm), (gq, gm) in zip(pairs, counts, got):
        assert int((cq >= thr).sum()) == nq and int(((cm >= thr) & vm).sum()) == nm
        eq, em = _expected_matches(pq.to(gpu), cq.to(gpu), pm.to(gpu), cm.to(gpu), vm.to(gpu), thr)
        assert np.array_equal(gq.cpu().numpy(), eq) and np.array_equal(gm.cpu().numpy(), em), (nq, nm)
        total += len(eq)
    assert total > 9 * 200


def test_run_pnp_batch_hands_all_64_bits_of_the_seed_to_the_kernel(gpu):
    from dust3r_amd.visloc.localization import PNP_SETTINGS, run_pnp_batch
    stats = []
    for case in seed_cases():
        assert (case['max_iters'], case['confidence']) == PNP_SETTINGS['cv2'] and case['thr'] == 5.0
        results, st = run_pnp_batch([(case['uv'], case['X'], K, None, 5.0)], seed=case['seed'], device=gpu, return_stats=True)
        abi, _, _ = pnp_abi([case], gpu)
        want = _same_rounds(case, abi[0])
        assert results[0][0] and st[0] == abi[0][2:] == (want['drawn'], want['best_h'])
        stats.append(st[0])
    assert seed_cases()[0]['seed'] == BIG_SEED == seed_cases()[1]['seed'] + 2 ** 63 and stats[0] != stats[1]     # the upper 32 bits matter
