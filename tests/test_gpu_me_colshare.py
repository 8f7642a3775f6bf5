"""GPU parity of the 8-bit full-search kernel that shares table column 2R over an MB's
qsad lanes (me.hip me_full_sad16_v7_kernel<R, G, true>; un-centred tables at range 16 and 8)
against the oracle's exhaustive search, on the shapes where its lane / wave / LDS layout
can go wrong: a wave with one live MB, MB counts that are no multiple of a wave's 8 or a
workgroup's 32 MBs, a wave spanning the frame boundary, content only column 2R sees, the
largest SADs, and the zeroed padding entries."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _search(hip, planes, origin, stride, mbw, mbh, nf, rng):
    """table[nf, mbh, mbw, 2R+1, P] (uint16, padding included) of fenc = planes[1:], ref = planes[:-1]"""
    dev = torch.from_numpy(planes).cuda()
    fs = planes[0].size
    table = hip.me_search_full(dev[1:], origin, stride, dev[:-1], origin, stride, mbw, mbh, nf, rng,
                               fenc_frame_stride=fs, ref_frame_stride=fs)
    return table.cpu().numpy().view(np.uint16)


def _check(hip, oracle, planes, origin, stride, mbw, mbh, nf, rng, padding=True):
    got = _search(hip, planes, origin, stride, mbw, mbh, nf, rng)
    assert got.shape[-1] == hip.me_table_pitch(rng)
    for f in range(nf):
        want = oracle.me_search_full(8, planes[f + 1].ravel(), origin, stride, planes[f].ravel(), origin, stride,
                                     mbw, mbh, rng)
        live = got[f][..., :2 * rng + 1]
        assert np.array_equal(live, want), f"frame {f}: {np.argwhere(live != want)[:5]}"
    if padding:
        assert not got[..., 2 * rng + 1:].any(), "entries 2R+1..P-1 must be zero"
    return got


# 1x1: a wave with one live MB; 5x3 x 2 frames: 30 MBs, a partly empty wave and one that
# spans the frame boundary; 9x1: one MB past a wave; 11x7: 77 MBs, more than two workgroups
@pytest.mark.parametrize("rng", [16, 8])
@pytest.mark.parametrize("mbw,mbh,nf", [(1, 1, 1), (5, 3, 2), (9, 1, 1), (11, 7, 1)])
def test_colshare_random(hip, oracle, mbw, mbh, nf, rng):
    from x264hip import synth
    planes, stride, origin = synth.random_planes(nf + 1, 16 * mbw, 16 * mbh, 8, seed=11 + mbw)
    _check(hip, oracle, planes, origin, stride, mbw, mbh, nf, rng)


@pytest.mark.parametrize("rng", [16, 8])
def test_colshare_synthetic(hip, oracle, rng):
    from x264hip import synth
    planes, stride, origin = synth.make_sequence(3, 80, 48, 8, seed=5)
    _check(hip, oracle, planes, origin, stride, 5, 3, 2, rng)


@pytest.mark.parametrize("rng", [16, 8])
@pytest.mark.parametrize("mbw,mbh", [(1, 2), (5, 3)])
def test_colshare_stripe(hip, oracle, mbw, mbh, rng):
    """ref is dark but for one bright pixel column per MB at x = 16 mbx + R + 15, the last pixel of
    window column 2R, which no other column of that MB's table reaches: a column 2R computed
    from column 2R-1's pixels (or not at all) differs by 16 * 255 in every row."""
    from x264hip import synth
    w, h = 16 * mbw, 16 * mbh
    stride = synth.plane_stride(w)
    origin = 32 * stride + 32
    rs = np.random.default_rng(2)
    ref = rs.integers(0, 8, size=(h + 64, stride)).astype(np.uint8)
    ref[:, 32 + rng + 15:32 + w + rng:16] = 255
    fenc = rs.integers(0, 8, size=(h + 64, stride)).astype(np.uint8)
    got = _check(hip, oracle, np.stack([ref, fenc]), origin, stride, mbw, mbh, 1, rng)[0]
    # the first MB column has no stripe to its left: it sees one in column 2R alone (the noise,
    # pixels 0..7, moves a column pair's difference by less than 256 * 7 of the stripe's 16 * 248)
    assert (got[:, 0, :, 2 * rng].astype(int) - got[:, 0, :, 2 * rng - 1] > 16 * 128).all()


@pytest.mark.parametrize("rng", [16, 8])
def test_colshare_extremes(hip, oracle, rng):
    """fenc all 0 against ref all 255: every entry is 256 * 255, column 2R included"""
    from x264hip import synth
    mbw, mbh = 5, 3
    stride = synth.plane_stride(16 * mbw)
    origin = 32 * stride + 32
    ref = np.full((16 * mbh + 64, stride), 255, np.uint8)
    got = _check(hip, oracle, np.stack([ref, np.zeros_like(ref)]), origin, stride, mbw, mbh, 1, rng)
    assert (got[..., :2 * rng + 1] == 65280).all()


def test_colshare_unaligned_plane(hip, oracle):
    """a plane pointer that is not dword aligned still takes the generic kernel and matches"""
    from x264hip import synth
    planes, stride, origin = synth.random_planes(3, 80, 48, 8, seed=4)
    _check(hip, oracle, planes, origin + 1, stride, 5, 3, 2, 16, padding=False)
