"""A handle's match configuration reaches every sub-handle family (GPU).

The single-handle `sgm_match_device` result is the reference; the same frames must come back
bit-identical through the per-device sub-handles (`sgm_match_batch`, `sgm_match_tiled`), the
same-device lanes of an OpenCV-mode batch (`sgm_match_device_batch`) and the band handles of
`sgm_match_tiled_exact`. Each configuration differs from a freshly created handle's in a field
that only a copied configuration carries (4 census paths, non-default BM parameters, another
mode), so a sub-handle left at its defaults gives another image.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, D = 128, 64, 32
N = 3
SEED = 0
BM = dict(texture_threshold=25, prefilter_size=7)
# The 9x9 texture sums of synth.py's blurred-noise pairs lie in about 850 .. 2450 (median 2200,
# tests/bm_reference.py sad_volume, seeds 0 .. 59), so no seed makes a threshold of 25 give another
# image than the default 10, and the pre-filter size is validated but unused by the X-Sobel
# pre-filter: the case above cannot see a BM copy that was missed. "bm_tex" is the same case with
# the threshold at the median texture, which rejects about half of the pixels.
BM_TEX = dict(texture_threshold=2200, prefilter_size=7)


@pytest.fixture(scope="module")
def frames(synth):
    return [synth.stereo_pair(H, W, 0, D, seed=SEED + i)[:2] for i in range(N)]


@pytest.fixture()
def eng(pkg):
    e = pkg.Engine(0)
    yield e
    e.close()


def _configure(pkg, eng, name):
    if name == "census4":
        eng.set_params(pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D))
        eng.set_census_paths(4)
    elif name == "census8":
        eng.set_params(pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D))
    elif name in ("bm", "bm_tex"):
        eng.set_params(pkg.default_params(pkg.MODE_OCV_BM, num_disparities=D, block_size=9))
        eng.set_bm_params(pkg.default_bm_params(**(BM if name == "bm" else BM_TEX)))
    else:
        eng.set_params(pkg.default_params(pkg.MODE_OCV_SGBM5, num_disparities=D))


def _match_device(torch, eng, left, right):
    dl, dr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    out = torch.full((H, W), 777, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    eng.match_device(dl.data_ptr(), dr.data_ptr(), W, H, W, out.data_ptr(), W)
    eng.synchronize()
    return out.cpu().numpy()


def _match_device_batch(torch, eng, frames):
    dl = [torch.from_numpy(f[0]).cuda() for f in frames]
    dr = [torch.from_numpy(f[1]).cuda() for f in frames]
    out = torch.full((len(frames), H, W), 777, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    eng.match_device_batch([t.data_ptr() for t in dl], [t.data_ptr() for t in dr], W, H, W,
                           [out[i].data_ptr() for i in range(len(frames))], W)
    eng.synchronize()
    return out.cpu().numpy()


def _same(got, ref, what):
    assert np.array_equal(got, ref), f"{what}: {int((got != ref).sum())} pixels differ from sgm_match_device"


def test_bm_case_distinguishes(pkg, eng, frames):
    """The "bm_tex" case gives another disparity image at the default BM parameters, so a sub-handle
    that missed the copy cannot pass below."""
    torch = pytest.importorskip("torch")
    _configure(pkg, eng, "bm_tex")
    ref = _match_device(torch, eng, *frames[0])
    eng.set_bm_params(pkg.default_bm_params())
    assert not np.array_equal(_match_device(torch, eng, *frames[0]), ref)


@pytest.mark.parametrize("name", ["census4", "bm", "bm_tex", "sgbm5"])
def test_sub_handles_match_the_handle(pkg, eng, frames, monkeypatch, name):
    torch = pytest.importorskip("torch")
    _configure(pkg, eng, name)
    refs = [_match_device(torch, eng, l, r) for l, r in frames]
    assert any((r != refs[0][0, 0]).any() for r in refs), "constant reference images"
    # sub: one handle per device, host frames streamed through the rings
    got = eng.match_batch([f[0] for f in frames], [f[1] for f in frames], devices=[0])
    for i in range(N):
        _same(got[i], refs[i], f"{name} sgm_match_batch frame {i}")
    # sub: two bands with a halo of the whole frame, so each band matches the full frame
    _same(eng.match_tiled(*frames[0], 2, H, devices=[0]), refs[0], f"{name} sgm_match_tiled")
    if name != "census4":
        # par: the same-device lanes of an OpenCV-mode device batch
        monkeypatch.setenv("SGM_OCV_STREAMS", "2")
        got = _match_device_batch(torch, eng, frames)
        for i in range(N):
            _same(got[i], refs[i], f"{name} sgm_match_device_batch frame {i}")


def test_band_handles_match_the_handle(pkg, eng, frames):
    torch = pytest.importorskip("torch")
    _configure(pkg, eng, "census8")
    ref = _match_device(torch, eng, *frames[0])
    _same(eng.match_tiled_exact(*frames[0], 2, devices=[0]), ref, "sgm_match_tiled_exact")


def test_debug_census_path_leaves_the_path_count(pkg, eng, oracle, frames):
    """sgm_debug_census_path runs on the eight-slice layout whatever the handle's path count, and the
    handle keeps its own."""
    torch = pytest.importorskip("torch")
    left, right = frames[0]
    _configure(pkg, eng, "census4")
    ref = _match_device(torch, eng, left, right)
    p = eng.get_params()
    op = oracle.make_params(oracle.MODE_CENSUS8, **{k: v for k, v in p.as_dict().items() if k != "mode"})
    assert np.array_equal(eng.census_path(left, right, 2), oracle.census_path(op, left, right, 2))
    assert eng.get_census_paths() == 4
    _same(_match_device(torch, eng, left, right), ref, "sgm_match_device after sgm_debug_census_path")


@pytest.mark.parametrize("entry", ["sgm_match_batch", "sgm_match_tiled", "sgm_match_tiled_device",
                                   "sgm_match_tiled_exact"])
def test_colour_frames_stay_refused(pkg, eng, frames, entry):
    torch = pytest.importorskip("torch")
    left, right = frames[0]
    _configure(pkg, eng, "census8")
    eng.set_raw_format(3, pkg.GRAY_Y14)
    with pytest.raises(pkg.SGMError) as ei:
        if entry == "sgm_match_batch":
            eng.match_batch([left], [right], devices=[0])
        elif entry == "sgm_match_tiled":
            eng.match_tiled(left, right, 2, H, devices=[0])
        elif entry == "sgm_match_tiled_exact":
            eng.match_tiled_exact(left, right, 2, devices=[0])
        else:
            dl, dr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
            out = torch.zeros((H, W), dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            eng.match_tiled_device(dl.data_ptr(), dr.data_ptr(), W, H, W, out.data_ptr(), W, 2, H, devices=[0])
    assert ei.value.code == pkg.SGM_ERR_UNSUPPORTED
    assert eng.error() == f"{entry} takes mono frames only (sgm_set_raw_format: 3 channels)"
