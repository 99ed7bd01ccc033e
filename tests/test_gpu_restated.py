"""The HIP path checked stage by stage against the numpy restatements (np_pipeline), not against the
oracle: normals, frames, sweep records and point lists, prune flags, images and scores, across the
parameter grid.  A misreading of the reference shared by the oracle and the kernels passes every
HIP-vs-oracle test; it fails here.  The same cases run on the oracle in test_oracle_restated.py.
"""
import pytest

import np_pipeline as npp
import restated_cases as rc

pytestmark = pytest.mark.gpu


def _detector(full):
    from agile_grasp2_amd import capi
    return capi.Detector(**full)


def _run(case, full):
    d = _detector(full)
    try:
        return npp.run(d, case)
    finally:
        d.close()


@pytest.mark.parametrize("seed", range(24))
def test_fuzz_configuration_restated(seed):
    """test_gpu_fuzz's 24 configurations (orientations 4..16, hand geometry, radii, both kinds of
    scene, filter_half_grasps 0 / 1)."""
    case, full = rc.fuzz_case(seed)
    rep = _run(case, full)
    rc.assert_reached(rep)
    if full["filter_half_grasps"] and rep["keep"].any():
        rc.expect_filter_half(rep)


@pytest.mark.parametrize("n_orient", [20, 32])
def test_many_orientations_restated(n_orient):
    """17..32 orientations: the sweep kernels' 32-slot instantiation."""
    case, full = rc.small_case(f"R{n_orient}", num_orientations=n_orient)
    rep = _run(case, full)
    rc.assert_reached(rep)
    assert rep["sweep"]["hyps"]["orientation"].max() >= 16


def test_filter_half_grasps_restated():
    case, full = rc.small_case("filter_half", filter_half_grasps=1)
    rep = _run(case, full)
    rc.assert_reached(rep)
    rc.expect_filter_half(rep)


def test_given_normals_restated():
    case, full = rc.given_normals_case()
    rep = _run(case, full)
    rc.assert_reached(rep)
    assert rep["normals"]["given"]


def test_xyz_samples_slot_base_restated():
    case, full = rc.xyz_samples_case()
    rep = _run(case, full)
    rc.assert_reached(rep)
    rc.expect_xyz_samples(rep, case)


def test_dense_unvoxelised_long_lists_restated():
    """Cropped lists of tens of thousands of points: the sweep's long-list stage (counted by
    n_overflow_samples) and lists of more staging chunks than the kept membership ballots."""
    case, full = rc.dense_case()
    rep = _run(case, full)
    rc.assert_reached(rep)
    assert rep["sweep"]["counters"].n_overflow_samples > 0
    rc.expect_dense(rep)


def test_two_cameras_restated():
    case, full = rc.two_camera_case()
    rep = _run(case, full)
    rc.assert_reached(rep)
    rc.expect_two_cameras(rep, case)


def test_prune_on_its_bounds():
    made = []

    def make(p):
        made.append(_detector(p))
        return made[-1]
    try:
        flips = rc.prune_on_bounds(make)
    finally:
        for d in made:
            d.close()
    assert {w[0] for w, _ in flips} == {"min_aperture", "max_aperture", "workspace", "min_z"}
    assert [e for _, e in flips].count(0) == 7 and [e for _, e in flips].count(1) == 9
