"""CPU: the claims of include/loik_amd_depth.h, proven on the numpy reference of tests/depth_numpy.py alone -- REPLACE is FUSE onto nothing,
a frame fused twice changes nothing, what the carve clears and keeps with the recommended band, the points win over the carve, every
return outside the padded robot ends in an occupied voxel, a robot rendered into its own image disappears with the recommended
filter_pad -- and, for every case the GPU tests use, that the ambiguous decisions stay within the cap."""
import numpy as np
import pytest

import depth_cases as DC
import depth_numpy as DN
import grid_numpy as GN

H = DC.H_EXACT


def _scene(seed=2100, size=(48, 36), dims=(40, 36, 28)):
    g = DC.camera("general", size)
    cam = DN.Camera(size[0], size[1], 40.0, 40.0, g.cx, g.cy, g.R, g.p, g.z_min, g.z_max)   # (a wide lens: the scene fills the image)
    img = DN.render(cam, spheres=[[1.2, 0.6, 0.5, 0.35]], boxes=[np.concatenate([DC.rot(2, 0.8, 0.6).reshape(9), [1.4, 1.5, 0.6], [0.2, 0.3, 0.25]])],
                    planes=[[0.6, 0.8, 0.0, 2.6]])
    origin = DC.grid_for(cam, dims, 0.05, ahead=0.4)
    return cam, img, dims, origin, 0.05


def test_replace_is_fuse_onto_an_empty_prior():
    cam, img, dims, origin, h = _scene()
    a = DN.integrate(cam=cam, depth=img, dims=dims, origin=origin, h=h, field=False)
    b = DN.integrate(cam=cam, depth=img, dims=dims, origin=origin, h=h, mode=DN.FUSE, prior=None, field=False)
    c = DN.integrate(cam=cam, depth=img, dims=dims, origin=origin, h=h, mode=DN.FUSE, carve_on=True, band=DN.COVER * h, prior=np.zeros(dims[::-1]), field=False)
    assert a["occ"].sum() > 50
    assert np.array_equal(a["occ"], b["occ"]) and np.array_equal(a["occ"], c["occ"]) and np.array_equal(a["stats"], b["stats"])


@pytest.mark.parametrize("band", [0.0, DN.COVER * 0.05])
def test_fusing_the_same_frame_twice_is_idempotent(band):
    cam, img, dims, origin, h = _scene()
    prior = GN.random_occupancy(dims, 0.05, 2101)
    kw = dict(cam=cam, depth=img, dims=dims, origin=origin, h=h, mode=DN.FUSE, carve_on=True, band=band, field=False)
    once = DN.integrate(prior=prior, **kw)
    twice = DN.integrate(prior=once["occ"], **kw)
    assert np.array_equal(once["occ"], twice["occ"])
    assert once["stats"][3] == twice["stats"][2] == twice["stats"][3]
    assert (prior != 0).sum() > once["occ"].sum() - once["stats"][1]   # something was carved


def test_a_wall_seen_head_on_clears_what_is_in_front_of_it_and_nothing_else():
    h = H
    cam = DN.Camera(33, 25, 64.0, 64.0, 16.0, 12.0, DC.LOOK_X, [-0.5, 0.25, 0.5], 0.25, 8.0)
    dims = (48, 40, 32)
    origin = DC.grid_for(cam, dims, h, ahead=0.25)
    wall_x = 1.515625   # world x of the wall, a quarter of a voxel into its layer: depth 2.015625
    img = DN.render(cam, planes=[[1.0, 0.0, 0.0, wall_x]])
    assert np.all(img == 2.015625)
    prior = np.ones(dims[::-1], dtype=np.uint8)
    res = DN.integrate(cam=cam, depth=img, dims=dims, origin=origin, h=h, mode=DN.FUSE, carve_on=True, band=DN.COVER * h, prior=prior, field=False)
    X, Y, Z = DN.centres_of(dims, origin, h)
    cv = DN.carve(prior, img, cam, dims, origin, h, DN.COVER * h)
    occ = res["occ"].astype(bool)
    hit = np.zeros_like(occ)
    ii = np.floor(DN.voxel_coords(res["points"][res["inside"]], origin, h)).astype(int)
    hit[ii[:, 2], ii[:, 1], ii[:, 0]] = True
    # cleared: exactly the voxels inside the image whose centre is more than the band in front of the wall, less those that hold a point
    front = (X + DN.COVER * h < wall_x)[None, None, :] & cv["inimg"]
    assert np.array_equal(~occ, front & ~hit) and front.sum() > 1000
    # a cleared voxel lies wholly in front of the wall: its far face is
    assert np.all((X + 0.5 * h)[np.nonzero(~occ)[2]] < wall_x)
    # kept: everything behind the wall, and everything outside the image
    assert occ[:, :, X > wall_x].all() and occ[~cv["inimg"]].all() and (~cv["inimg"]).sum() > 1000
    # band = 0 clears one layer more: the one whose centres are 0.75 h in front of the wall
    res0 = DN.integrate(cam=cam, depth=img, dims=dims, origin=origin, h=h, mode=DN.FUSE, carve_on=True, band=0.0, prior=prior, field=False)
    assert res0["occ"].sum() < res["occ"].sum()


def test_the_carve_never_clears_a_voxel_that_holds_a_point_of_the_frame():
    cam, img, dims, origin, h = _scene()
    res = DN.integrate(cam=cam, depth=img, dims=dims, origin=origin, h=h, mode=DN.FUSE, carve_on=True, band=0.0, prior=np.ones(dims[::-1]), field=False)
    ii = np.floor(DN.voxel_coords(res["points"][res["inside"]], origin, h)).astype(int)
    assert ii.shape[0] > 100 and res["occ"][ii[:, 2], ii[:, 1], ii[:, 0]].all()
    cleared = DN.carve(np.ones(dims[::-1]), img, cam, dims, origin, h, 0.0)["cleared"]
    assert cleared[ii[:, 2], ii[:, 1], ii[:, 0]].any()   # (the carve alone would have cleared some of them: the points win)


def test_every_return_outside_the_padded_robot_lies_in_an_occupied_voxel():
    cam, img, dims, origin, h = _scene()
    cen, rad, pad = np.array([[1.2, 0.6, 0.5], [1.0, 1.2, 0.6]]), np.array([0.3, 0.15]), DN.COVER * h
    res = DN.integrate(cam=cam, depth=img, dims=dims, origin=origin, h=h, filter_centres=cen, filter_radii=rad, filter_pad=pad, field=False)
    pts = res["points"][res["inside"]]
    ii = np.floor(DN.voxel_coords(pts, origin, h)).astype(int)
    X, Y, Z = DN.centres_of(dims, origin, h)
    ctr = np.stack([X[ii[:, 0]], Y[ii[:, 1]], Z[ii[:, 2]]], axis=1)
    outside = (np.linalg.norm(ctr[:, None] - cen[None], axis=2) > (rad + pad)[None]).all(axis=1)
    assert outside.sum() > 100 and (~outside).sum() > 10
    assert res["occ"][ii[outside, 2], ii[outside, 1], ii[outside, 0]].all()
    assert not res["occ"][ii[~outside, 2], ii[~outside, 1], ii[~outside, 0]].any()   # the filter wins over the points


def test_a_robot_rendered_into_its_own_image_is_free_with_the_recommended_pad():
    r = DC.robot()
    model, links, spheres, q = r["model"], r["links"], r["spheres"], r["q"][:1]
    cen = r["centres"][0]
    h = 0.04
    cam = DN.Camera(96, 72, 80.0, 80.0, 47.5, 35.5, DC.LOOK_X, [-1.6, 0.0, 0.4], 0.2, 6.0)
    img = DN.render(cam, spheres=np.concatenate([cen, spheres[:, 3:]], axis=1), planes=[[1.0, 0.0, 0.0, 1.4]])
    dims = (72, 64, 56)
    origin = np.array([-1.2, -1.28, -0.7]) + 1.0 / 8192.0
    kw = dict(cam=cam, depth=img, dims=dims, origin=origin, h=h, field=False)
    raw = DN.integrate(**kw)
    seen = DN.integrate(filter_centres=cen, filter_radii=spheres[:, 3], filter_pad=DN.COVER * h, **kw)
    for res in (raw, seen):   # (thousands of occupied voxels: the field by the three passes, which test_grid_numpy.py proves equal to the brute force)
        res["G"] = GN.field_passes(res["occ"])
    clr = lambda res: GN.clearance(model, q, links, spheres, grid=GN.Grid(res["occ"], origin, h, G=res["G"]))["min"][0]
    assert clr(raw) <= 0.0 < clr(seen)
    assert seen["occ"].sum() > 100   # the wall behind the robot stays
    # ... and the exact distance to the cubes that remain is positive too
    assert GN.exact_clearance(model, q, links, spheres, GN.Grid(seen["occ"], origin, h, G=seen["G"]))[0] > 0.0


@pytest.mark.parametrize("name", list(DC.CASES))
def test_the_cases_of_the_gpu_tests_stay_within_the_cap(name):
    c = DC.case(name)
    for mode in ("replace", "fuse"):
        res = c[mode]
        for step, (amb, n) in res["ambiguous"].items():
            print("depth_measured %s %s %s: %d ambiguous of %d decisions" % (name, mode, step, amb, n))
            # (the cap is for the general cases.  In an exact case a voxel's centre may project exactly onto a pixel boundary: the arithmetic
            # is exact there, so the decision is the same on both sides)
            assert c["kind"] == "exact" or amb <= DC.CAP * max(n, 1), (name, mode, step, amb, n)
        if c["kind"] == "exact":
            assert res["ambiguous"]["points"][0] == 0 and res["ambiguous"].get("filter", (0, 0))[0] == 0
    assert c["replace"]["stats"][0] > 0 and c["replace"]["stats"][1] > 0, name
    if c["nf"]:
        plain = DN.integrate(cam=c["cam"], depth=c["img"], dims=c["dims"], origin=c["origin"], h=c["h"], field=False)
        print("depth_measured %s: the filter clears %d voxels" % (name, int(plain["occ"].sum() - c["replace"]["occ"].sum())))
    if name != "general-1x1-one" and "one" not in name:
        assert c["fuse"]["stats"][2] > c["fuse"]["stats"][3] - c["fuse"]["stats"][1], name   # the carve cleared something
