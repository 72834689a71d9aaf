"""The newer stages of the C++ mirror -- paris::weight()'s scatter, phase-retrieval, beam-hardening and metal branches (paris/stages.h),
and the paris::hip functions behind them, the metal reinsertion, the bilateral filter and the pieces of the beam-hardening fit
(paris/hip/backend.h) -- against the Python Backend's chain, bit for bit on uint32 views. paris_hip_demo runs the loop with the flags
that map onto the mirror's setters; paris_hip_mirror_calls makes the calls no loop reaches. Beside every equality stands a reference that
is deliberately wrong in the way a wrapper could be -- passes in another order, another view's trace, a slab offset of 0, exchanged
sigmas, halves without their halo -- and the assertion that it differs, so the inputs are shown to tell the misreading apart."""
import os
import subprocess

import numpy as np
import pytest

import binning_rule as BR
import chain_rule as CH
import grid_cap_rule
import metal_rule as R
import test_beam_hardening_host as BHH
import test_gpu_flat_field as FF
import test_gpu_metal_driver as MD
from paris_amd import _lib
from paris_amd import backend as B
from test_gpu_chain_driver import EXTEND, mirror_volume, write_scan
from test_gpu_phase_driver import ETA, alpha_for
from test_gpu_scatter_driver import PHASE_MARGIN, mirror, setting_for

pytestmark = pytest.mark.gpu

N = CH.N_FRAMES
K = 17                                  # --clear-after: the passes act on the frames 0 .. 17 of 36
DEMO = FF.DEMO
CALLS = os.path.join(os.path.dirname(DEMO), "paris_hip_mirror_calls")
BUILDS = ("", "_immediate", "_serial", "_snapshots", "_filter_at_once", "_upload_stream")
INVALID = _lib.load().paris_hip_strerror(_lib.ERROR_INVALID_ARGUMENT).decode()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def run(exe, args, ok=True):
    """one run of a program of paris_amd/host/demo: (stdout, stderr); ok False: it must end with status 1"""
    r = subprocess.run([str(a) for a in [exe] + list(args)], capture_output=True, text=True, timeout=300)
    if r.returncode < 0:                # killed by a signal: nothing more is started on a device that may have faulted
        pytest.exit("%s died of signal %d\n%s" % (exe, -r.returncode, r.stdout + r.stderr), returncode=3)
    assert r.returncode == (0 if ok else 1), (r.returncode, r.stdout + r.stderr)
    return r.stdout, r.stderr


def demo(root, geo, n, frames, out, flags, build="", ok=True):
    """paris_hip_demo on root/frames into root/out: the volume as a flat array, or stderr where the run must be refused -- and then it
    must have written nothing"""
    path = root / out
    if path.exists():
        path.unlink()
    _, err = run(DEMO + build, [v for v in geo] + [n, root / frames, path] + list(flags), ok)
    if not ok:
        assert not path.exists(), "a refused run wrote " + out
        return err
    return np.fromfile(path, np.float32)


# ---- the chain's scan ----------------------------------------------------------------------------------------------------------------

def chain_flags(root, st, rings=True):
    """--flat --air-region --defects --zingers [--rings] as tests/test_gpu_chain_driver.py gives them to the demo"""
    tag = "_%d.raw" % st.bin
    flags = ["--flat", root / ("dark" + tag), root / ("flat" + tag), "%.9g" % st.t_min, "--air-region"] + list(st.rect) + [
        0, "--defects", root / ("mask" + tag), "--zingers", "%.9g" % st.zingers[0], "%.9g" % st.zingers[1], st.zingers[2]]
    return flags + (["--rings", st.rings[0], "%.9g" % st.rings[1], "%.9g" % st.rings[2]] if rings else [])


def scatter_flags(setting):
    return ["--scatter"] + ["%.9g" % v for v in setting[:7]] + list(setting[7:])


def phase_flags(st):
    return ["--phase-alpha", "%.9g" % alpha_for(st), "%.9g" % st.t_min, PHASE_MARGIN]


def bh_flags(st):
    return ["--beam-hardening", "%.9g:%.9g" % st.bh]


def write_settings(root, st):
    tag = "_%d.raw" % st.bin
    np.ascontiguousarray(st.dark, np.float32).tofile(root / ("dark" + tag))
    np.ascontiguousarray(st.flat, np.float32).tofile(root / ("flat" + tag))
    st.mask.tofile(root / ("mask" + tag))


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """CH.scan() with --defects alone, as test_the_cpp_mirror_equals_the_driver sets it, and the same scan for --bin 2 2 none: no source
    mask, the references binned by the numpy rule, the map of the binned detector"""
    root = tmp_path_factory.mktemp("mirror_stages")
    s = CH.scan()
    st = CH.settings(s, 1)
    st.mask = (s.mask != 0).astype(np.uint8)
    st.plan = B.defect_plan(st.mask)
    write_scan(root, s)
    s.counts.astype(np.float32).tofile(root / "in.raw")
    write_settings(root, st)
    b2 = CH.settings(s, 2)
    b2.src_mask = None
    b2.dark, b2.flat = BR.bin_frame(s.dark, 2, 2, None), BR.bin_frame(s.flat, 2, 2, None)
    b2.mask = ((b2.mask != 0) | (CH.dead_pixels(b2.dark, b2.flat) != 0)).astype(np.uint8)
    b2.plan = B.defect_plan(b2.mask)
    write_settings(root, b2)
    everything = (chain_flags(root, st) + scatter_flags(setting_for(st)) + phase_flags(st) + bh_flags(st)
                  + ["--detector-roll", "%.9g" % ETA, "--extend-rows", EXTEND[0], EXTEND[1]])
    return dict(root=root, s=s, st=st, b2=b2, everything=everything, cache={})


def reference(chain, name, make):
    """a volume of the Python chain, computed once for the tests that share it and never changed"""
    if name not in chain["cache"]:
        v = make()
        v.setflags(write=False)
        chain["cache"][name] = v
    return chain["cache"][name]


def everything_set(chain, **how):
    s, st = chain["s"], chain["st"]
    return mirror(s, st, setting_for(st), alpha_for(st), extend=EXTEND, **how)


def want_of_a(chain):
    return reference(chain, "a", lambda: everything_set(chain))


# ---- a. the order of the frame chain, b. in every build -----------------------------------------------------------------------------

WRONG_ORDERS = {"scatter and phase swapped": ("phase", "scatter", "beam_hardening", "roll"),
                "beam hardening in front of the scatter correction": ("beam_hardening", "scatter", "phase", "roll"),
                "the roll in front of beam hardening": ("scatter", "phase", "roll", "beam_hardening")}


@pytest.mark.parametrize("wrong", sorted(WRONG_ORDERS))
def test_the_scan_tells_the_orders_apart(chain, wrong):
    want = want_of_a(chain)
    assert np.abs(want).max() > 0 and np.isfinite(want).all()
    assert not same(everything_set(chain, order=WRONG_ORDERS[wrong]), want), wrong


@pytest.mark.parametrize("build", BUILDS)
def test_weight_runs_the_new_passes_in_the_documented_order(chain, build):
    """--flat --air-region --defects --zingers --rings --scatter --phase-alpha --beam-hardening --detector-roll --extend-rows --slabs 2:
    the Python chain with scatter then phase between ring_correct_rows and beam_hardening, the roll behind them, then weight, filter
    with the row extension and backproject -- in the deferred default build and in each A/B build of the host Makefile"""
    want = want_of_a(chain)
    got = demo(chain["root"], CH.GEO, N, "in.raw", "a%s.raw" % build, chain["everything"] + ["--slabs", 2], build)
    assert got.size == want.size and same(got.reshape(want.shape), want), build or "paris_hip_demo"


# ---- c. each new branch alone --------------------------------------------------------------------------------------------------------

def branch(chain, st, name, rings):
    how = dict(scatter=setting_for(st) if name == "scatter" else None, alpha=alpha_for(st) if name == "phase" else None,
               beam_hardening=name == "beam_hardening")
    return reference(chain, "%s_%d" % (name, st.bin), lambda: mirror(chain["s"], st, how["scatter"], how["alpha"], rings=rings, roll=None,
                                                                     beam_hardening=how["beam_hardening"]))


BRANCH_FLAGS = {"scatter": lambda st: scatter_flags(setting_for(st)), "phase": phase_flags, "beam_hardening": bh_flags, "none": lambda st: []}


@pytest.mark.parametrize("slabs", [1, 3])
@pytest.mark.parametrize("name", ["scatter", "phase", "beam_hardening"])
def test_each_new_branch_alone(chain, name, slabs):
    st = chain["st"]
    want, plain = branch(chain, st, name, True), branch(chain, st, "none", True)
    got = demo(chain["root"], CH.GEO, N, "in.raw", "c.raw", chain_flags(chain["root"], st) + BRANCH_FLAGS[name](st) + ["--slabs", slabs])
    assert np.abs(want).max() > 0 and not same(want, plain)
    assert got.size == want.size and same(got.reshape(want.shape), want)
    assert not same(got.reshape(want.shape), plain)


@pytest.mark.parametrize("name", ["scatter", "phase", "beam_hardening"])
def test_each_new_branch_with_bin_2_takes_the_binned_detector_s_size_and_pitches(chain, name):
    """--bin 2 2 none (which the demo refuses with --rings): the setters get 33 x 22 pixels of twice the pitch"""
    st = chain["b2"]
    assert (st.dim_x, st.dim_y) == (33, 22) and st.geo[2] == 2 * CH.GEO[2]
    want, plain = branch(chain, st, name, False), branch(chain, st, "none", False)
    got = demo(chain["root"], CH.GEO, N, "in.raw", "c2.raw",
               ["--bin", 2, 2, "none"] + chain_flags(chain["root"], st, rings=False) + BRANCH_FLAGS[name](st) + ["--slabs", 2])
    assert np.abs(want).max() > 0 and not same(want, plain)
    assert got.size == want.size and same(got.reshape(want.shape), want)


# ---- f. clear -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("slabs", [1, 2])
def test_clear_after_k_and_the_set_at_the_top_of_the_next_slab(chain, slabs):
    """the passes on the frames 0 .. K, the rest without them; in two slabs the second one has them set again"""
    want = reference(chain, "clear", lambda: everything_set(chain, last=K))
    none = reference(chain, "clear_at_once", lambda: mirror(chain["s"], chain["st"], None, None, beam_hardening=False, extend=EXTEND))
    assert not same(want, want_of_a(chain)) and not same(want, none)
    got = demo(chain["root"], CH.GEO, N, "in.raw", "f.raw", chain["everything"] + ["--clear-after", K, "--slabs", slabs])
    assert got.size == want.size and same(got.reshape(want.shape), want)


# ---- g. refusals ---------------------------------------------------------------------------------------------------------------------

def test_a_refused_setting_ends_the_run(chain):
    root, st = chain["root"], chain["st"]
    base = chain_flags(root, st)
    err = demo(root, CH.GEO, N, "in.raw", "g.raw", base + scatter_flags(setting_for(st, limit=1.5)), ok=False)
    assert "pipeline execution failed: set_scatter_correction() failed: " + INVALID in err, err
    err = demo(root, CH.GEO, N, "in.raw", "g.raw", base + ["--phase-alpha", "%.9g" % alpha_for(st), "%.9g" % st.t_min, 0], ok=False)
    assert "pipeline execution failed: set_phase_retrieval() failed: " + INVALID in err, err
    err = demo(root, CH.GEO, N, "in.raw", "g.raw", base + ["--beam-hardening", "0.93:0.11:0.01:0.001:0.0001"], ok=False)
    assert "pipeline execution failed: set_beam_hardening() failed: " + INVALID in err, err
    got = demo(root, CH.GEO, N, "in.raw", "g.raw", base + bh_flags(st))          # and the valid setting then works
    assert same(got, branch(chain, st, "beam_hardening", True).ravel())


def test_a_refused_setting_is_not_recorded_for_the_thread(chain, tmp_path):
    """in ONE process (a following run of the demo starts with empty sets whatever the setter did): each of the four setters throws,
    and paris::weight() afterwards is the plain cosine weight -- a has_*() that answered yes would send the frame into a pass the
    library has no setting for, and the run would end with its refusal"""
    det = B.DetectorGeometry(*CH.GEO)
    frame = np.ascontiguousarray(chain["s"].lines[3], np.float32)
    frame.tofile(tmp_path / "in.raw")
    with B.Backend(0) as be:
        d_p = B.load(be, B.Projection(frame.copy(), det.n_row, det.n_col, idx=0))
        B.weight(be, d_p, det)
        h = be.make_projection_host(det.n_row, det.n_col)
        be.copy_d2h(d_p, h)
        want = h.buf.copy()
        be.free(d_p)
    run(CALLS, ["refused"] + list(CH.GEO) + [tmp_path / "in.raw", tmp_path / "out.raw"])
    assert not np.array_equal(bits(want), bits(frame)) and same(np.fromfile(tmp_path / "out.raw", np.float32), want.ravel())


# ---- d. metal -------------------------------------------------------------------------------------------------------------------------

VIEWS = R.SCENE_VIEWS
METAL_K = 59                            # of 120 views


@pytest.fixture(scope="module")
def metal(tmp_path_factory):
    root = tmp_path_factory.mktemp("mirror_metal")
    _, _, frames = MD.scene_scan()
    np.ascontiguousarray(frames, np.float32).tofile(root / "in.raw")
    volume, mt, _ = MD.python_chain(frames, True)
    assert mt.bits.shape == (VIEWS, MD.DET.n_col, 1) and len(mt.index) > 100 and mt.trace_pixels > 0
    write_trace(root, "", mt)
    return dict(root=root, frames=frames, want=volume, mt=mt)


def write_trace(root, tag, mt):
    np.ascontiguousarray(mt.bits, np.uint64).tofile(root / ("bits%s.raw" % tag))
    np.ascontiguousarray(mt.index, np.uint64).tofile(root / ("index%s.raw" % tag))
    np.ascontiguousarray(mt.value, np.float32).tofile(root / ("value%s.raw" % tag))


def metal_flags(root, tag="", voxels=True):
    return ["--metal-trace", root / ("bits%s.raw" % tag), VIEWS] + (
        ["--metal-voxels", root / ("index%s.raw" % tag), root / ("value%s.raw" % tag)] if voxels else [])


def reinserted(volume, mt, slabs, offset_of):
    """numpy: the listed voxels put into each of `slabs` slabs of the volume, slab k taken for slices [offset_of(k), ...) of the grid"""
    out = np.array(volume, np.float32)
    dz = out.shape[0] // slabs
    plane = out.shape[1] * out.shape[2]
    for k in range(slabs):
        slab = out[k * dz:out.shape[0] if k == slabs - 1 else (k + 1) * dz].reshape(-1)      # a view: the slab's slices are contiguous
        local = mt.index.astype(np.int64) - offset_of(k) * plane
        inside = (local >= 0) & (local < slab.size)
        slab[local[inside]] = mt.value[inside]
    return out


@pytest.mark.parametrize("slabs", [1, 3])
def test_metal_trace_and_voxels(metal, slabs):
    """set_metal_trace, metal_inpaint with p.idx as the view, set_metal_voxels and metal_reinsert at the slab's offset"""
    want, mt = metal["want"], metal["mt"]
    got = demo(metal["root"], R.SCENE_DET, VIEWS, "in.raw", "d.raw", metal_flags(metal["root"]) + ["--slabs", slabs])
    assert np.abs(want).max() > 0 and got.size == want.size and same(got.reshape(want.shape), want)


def test_the_scene_tells_the_metal_misreadings_apart(metal):
    frames, want, mt = metal["frames"], metal["want"], metal["mt"]
    assert not same(MD.python_chain(frames, True, view=lambda i: 0)[0], want), "view 0 for every frame"
    assert not same(MD.python_chain(frames, True, view=lambda i: (i + 1) % VIEWS)[0], want), "view i + 1"
    bare = MD.python_chain(frames, True, reinsert=False)[0]
    dz = want.shape[0] // 3
    assert same(reinserted(bare, mt, 3, lambda k: k * dz), want)                  # the numpy statement of the reinsertion holds ...
    assert not same(reinserted(bare, mt, 3, lambda k: 0), want), "v_offset 0 in every slab"


def test_metal_with_the_roll_and_the_zinger_filter(metal):
    """as tests/test_gpu_metal_driver.py combines them: the trace lives on the detector the roll writes"""
    root = metal["root"]
    want, mt, _ = MD.python_chain(metal["frames"], True, roll=MD.ROLL, zingers=MD.ZINGERS)
    write_trace(root, "_roll", mt)
    got = demo(root, R.SCENE_DET, VIEWS, "in.raw", "d_roll.raw", metal_flags(root, "_roll") + [
        "--detector-roll", "%.9g" % MD.ROLL, "--zingers", "%.9g" % MD.ZINGERS[0], "%.9g" % MD.ZINGERS[1], 0, "--slabs", 3])
    assert not same(want, metal["want"]) and got.size == want.size and same(got.reshape(want.shape), want)


@pytest.mark.parametrize("slabs", [1, 3])
def test_clear_metal_trace_after_k(metal, slabs):
    """the frames 0 .. K inpainted, the others not (and nothing reinserted: no --metal-voxels); each slab sets the trace again"""
    if "clear" not in metal:
        metal["clear"] = MD.python_chain(metal["frames"], True, reinsert=False, last=METAL_K)[0]
        metal["bare"] = MD.python_chain(metal["frames"], True, reinsert=False)[0]
        metal["none"] = MD.python_chain(metal["frames"], False)[0]
    want = metal["clear"]
    assert not same(want, metal["bare"]) and not same(want, metal["none"])
    got = demo(metal["root"], R.SCENE_DET, VIEWS, "in.raw", "d_clear.raw",
               metal_flags(metal["root"], voxels=False) + ["--clear-after", METAL_K, "--slabs", slabs])
    assert got.size == want.size and same(got.reshape(want.shape), want)


def test_cleared_metal_voxels_are_gone_and_a_trace_of_another_width_is_refused(metal, tmp_path):
    """after clear_metal_voxels() the library has no list: metal_reinsert() refuses. And a trace file packed for a detector of 67
    pixels a row -- two words a row where 64 pixels have one -- is not taken for this detector's."""
    root = metal["root"]
    _, err = run(DEMO, list(R.SCENE_DET) + [VIEWS, root / "in.raw", tmp_path / "out.raw"] + metal_flags(root) + ["--clear-after", METAL_K], ok=False)
    assert "pipeline execution failed: metal_reinsert() failed: " + INVALID in err, err
    np.zeros((VIEWS, MD.DET.n_col, B.metal_words(67)), np.uint64).tofile(root / "bits_67.raw")
    err = demo(root, R.SCENE_DET, VIEWS, "in.raw", "d_67.raw", ["--metal-trace", root / "bits_67.raw", VIEWS], ok=False)
    assert "pipeline execution failed: cannot read " + str(root / "bits_67.raw") in err, err


# ---- e. denoise ----------------------------------------------------------------------------------------------------------------------

SIGMA_S = 1.5


@pytest.fixture(scope="module")
def plain_volume(tmp_path_factory):
    """the plain chain: the scan's line integrals through weight, filter and backprojection"""
    root = tmp_path_factory.mktemp("mirror_denoise")
    s = CH.scan()
    s.lines.tofile(root / "in.raw")
    with B.Backend(0) as be:
        v, _, _ = mirror_volume(be, s.lines, s.geo)
    return root, v, float(np.float32(0.1 * np.abs(v).max()))


def bilateral(v, sigma_r, sigma_s, radius, parts=((0, None, 0, None),)):
    """Backend.volume_bilateral of the host volume v; parts: (source first, source end, z_first, z_count) -- one call each, the results
    one behind the other"""
    out = []
    with B.Backend(0) as be:
        be.set_volume_bilateral(sigma_r, sigma_s, radius)
        for first, end, z_first, z_count in parts:
            src = np.ascontiguousarray(v[first:end])
            d_v = be.make_volume_device(src.shape[2], src.shape[1], src.shape[0])
            be.copy_h2d(B.Volume(src, src.shape[2], src.shape[1], src.shape[0]), d_v)
            d_o = be.volume_bilateral(d_v, z_first=z_first, z_count=z_count)
            h = be.make_volume_host(d_o.dim_x, d_o.dim_y, d_o.dim_z)
            be.copy_d2h(d_o, h)
            out.append(h.buf.reshape(d_o.dim_z, d_o.dim_y, d_o.dim_x).copy())
            be.free(d_o)
            be.free(d_v)
    return np.concatenate(out)


@pytest.mark.parametrize("radius", [1, 3])
def test_denoise_in_two_ranges_equals_one_call(plain_volume, radius):
    root, v, sigma_r = plain_volume
    want = bilateral(v, sigma_r, SIGMA_S, radius)
    h = v.shape[0] // 2
    assert h > radius and not same(want, v)
    assert not same(bilateral(v, SIGMA_S, sigma_r, radius), want), "sigma_r and sigma_s exchanged"
    assert not same(bilateral(v, sigma_r, SIGMA_S, radius, ((0, h, 0, None), (h, None, 0, None))), want), "each half from its own slices only"
    got = demo(root, CH.GEO, N, "in.raw", "e.raw", ["--denoise", "%.9g" % sigma_r, "%.9g" % SIGMA_S, radius])
    assert got.size == want.size and same(got.reshape(want.shape), want)


# ---- h. the pieces of the beam-hardening fit -----------------------------------------------------------------------------------------

BH_DIMS = (13, 11, 7)                   # odd: 1001 voxels
BH_THR, BH_MARGIN = 0.5, 0
BH_BINS, BH_RANGE = 64, (-8.0, 8.0)


@pytest.mark.parametrize("degree", [2, 4])
def test_mirror_calls_bh(tmp_path, degree):
    dim_x, dim_y, dim_z = BH_DIMS
    basis, _ = BHH.gram_case(dim_x * dim_y * dim_z, degree, seed=degree)
    hist = np.histogram(basis[0][np.isfinite(basis[0])], BH_BINS, BH_RANGE)[0].astype(np.uint64)
    for k, f in enumerate(basis):
        f.tofile(tmp_path / ("f_%d.raw" % k))
    hist.tofile(tmp_path / "hist.raw")
    with B.Backend(0) as be:
        vols = []
        for f in basis:
            vols.append(be.make_volume_device(dim_x, dim_y, dim_z))
            be.copy_h2d(B.Volume(np.ascontiguousarray(f.reshape(dim_z, dim_y, dim_x)), dim_x, dim_y, dim_z), vols[-1])
        d_l = be.bh_classify(vols[0], BH_THR, BH_MARGIN)
        labels = be.labels_to_host(d_l)
        gram, counts = be.bh_gram(vols, d_l)
    fit = B.bh_solve(gram, degree, counts)
    thr = B.bh_threshold_from_histogram(hist, *BH_RANGE)
    assert {0, 1, 2} == set(np.unique(labels)) and counts.n_object > 50 and counts.n_air > 50 and counts.n_ignored > 50
    run(CALLS, ["bh", dim_x, dim_y, dim_z, BH_THR, BH_MARGIN, degree] + [tmp_path / ("f_%d.raw" % k) for k in range(degree)] + [
        tmp_path / "hist.raw", BH_RANGE[0], BH_RANGE[1], tmp_path / "out"])
    assert np.array_equal(np.fromfile(tmp_path / "out.labels", np.uint8), labels.ravel())
    assert np.array_equal(np.fromfile(tmp_path / "out.gram", np.uint64), gram.view(np.uint64))
    assert tuple(np.fromfile(tmp_path / "out.counts", np.uint64)) == (counts.n_object, counts.n_air, counts.n_ignored, counts.n_not_finite)
    fitted = np.array([fit.setting.degree] + [float(c) for c in fit.setting.c] + [fit.level, fit.residual_before, fit.residual_after], np.float64)
    assert fit.setting.degree == degree and np.array_equal(np.fromfile(tmp_path / "out.fit", np.uint64), fitted.view(np.uint64))
    assert np.array_equal(np.fromfile(tmp_path / "out.threshold", np.uint32), np.array([thr], np.float32).view(np.uint32))
    assert BH_RANGE[0] < thr < BH_RANGE[1]


# ---- i. two frames of three ----------------------------------------------------------------------------------------------------------

GAP_ROWS = 3


@pytest.mark.parametrize("what", ["scatter", "phase"])
def test_mirror_calls_frames(chain, tmp_path, what):
    """scatter_correction / phase_retrieval on two of three frames in one pitched buffer whose frame stride holds GAP_ROWS more rows
    than a frame: the third frame and the rows between keep every bit"""
    st = chain["st"]
    dim_x, dim_y = st.dim_x, st.dim_y
    sentinel = grid_cap_rule.SENTINEL
    lines = reference(chain, "lines", lambda: CH.chain(chain["s"].counts[:3], st, upto=2)[0][2])       # line integrals of three frames
    before = np.full((3, dim_y + GAP_ROWS, dim_x), sentinel, np.uint32).view(np.float32)
    before[:, :dim_y] = lines
    before.tofile(tmp_path / "in.raw")
    setting = setting_for(st)
    with B.Backend(0) as be:
        owner = be.make_projection_device(dim_x, 3 * (dim_y + GAP_ROWS))
        be.upload_raw(before.reshape(-1, dim_x), owner)
        p = be.wrap_projection(owner.ptr, owner.pitch, dim_x, dim_y)
        at = dict(frame_stride=owner.pitch * (dim_y + GAP_ROWS), n_frames=2)
        if what == "scatter":
            be.set_scatter_correction(setting, dim_x, dim_y, st.geo[2], st.geo[3])
            be.scatter_correction(p, **at)
        else:
            be.set_phase_retrieval(alpha_for(st), st.t_min, PHASE_MARGIN, dim_x, dim_y, st.geo[2], st.geo[3])
            be.phase_retrieval(p, **at)
        h = be.make_projection_host(dim_x, 3 * (dim_y + GAP_ROWS))
        be.copy_d2h(owner, h)
        want = h.buf.reshape(before.shape).copy()
        be.free(owner)
    assert not np.array_equal(bits(want[:2, :dim_y]), bits(before[:2, :dim_y]))
    assert np.array_equal(bits(want[2]), bits(before[2])) and np.all(bits(want[:, dim_y:]) == sentinel)
    run(CALLS, ["frames", dim_x, dim_y, "%.9g" % st.geo[2], "%.9g" % st.geo[3], GAP_ROWS, tmp_path / "in.raw", tmp_path / "out.raw", what]
        + (scatter_flags(setting)[1:] if what == "scatter" else phase_flags(st)[1:]))
    got = np.fromfile(tmp_path / "out.raw", np.float32).reshape(before.shape)
    assert np.array_equal(bits(got[:2, :dim_y]), bits(want[:2, :dim_y])), "the two frames"
    assert np.array_equal(bits(got[2]), bits(before[2])), "the third frame"
    assert np.all(bits(got[:, dim_y:]) == sentinel), "the rows between the frames"
