"""The shared NHWC max-pool (kernels.hip maxpool_kernel) in its two 3 x 3 forms, taken from inside the networks that run it, and the
two writers of the static CNN's zero-bordered image (preprocess_kernel from u8 frames, pack_nchw_kernel from the preprocessed tensor).
The pool is compared exactly: a maximum of stored values is one of them in every storage.  Its 2 x 2 form is pinned by
test_gpu_s3fd.py::test_maxpool2_is_exact and test_gpu_sp32_pairs.py::test_maxpool2_sp32_identity_writes_the_python_pair."""
import pytest
import torch
import torch.nn.functional as F

from avcer_amd import synth
from avcer_amd.engine import MODE_BF16, MODE_F16X3, MODE_FP32
from oracle import video as ov

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine_face(engine):
    engine.load_face(synth.to_torch(synth.retina_state_dict(42)))
    return engine


def _tap(forward, eng, name, shape, mode):
    """One debug tap of `forward` as f32 NHWC `shape`: f32 storage as it is, bf16 storage widened (exact)."""
    bf = mode == MODE_BF16
    numel = shape[0] * shape[1] * shape[2] * shape[3]
    dst = eng.debug_tap(name, numel, dtype=torch.int16 if bf else torch.float32)
    forward()
    torch.cuda.synchronize()
    assert eng.debug_tap_copied() == numel * (2 if bf else 4), name
    got = dst.cpu()
    if bf:
        got = (got.to(torch.int32) << 16).view(torch.float32)
    return got.view(shape)


def _pool_ref(x_nhwc, pad):
    return F.max_pool2d(x_nhwc.permute(0, 3, 1, 2), 3, 2, pad).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("mode", [MODE_FP32, MODE_BF16])
def test_static_stem_pool_is_the_maximum_of_its_window(engine_static, mode):
    """video.py:103 MaxPool2d(3, 2) without padding: 112 x 112 -> 55 x 55, the last row and column of the input unread."""
    frames = torch.from_numpy(synth.face_frames(1234, 1))
    run = lambda: engine_static.static_forward(frames, mode)
    conv = _tap(run, engine_static, "stem_conv", (1, 112, 112, 64), mode)
    pool = _tap(run, engine_static, "stem", (1, 55, 55, 64), mode)
    assert conv.abs().max() > 0 and torch.equal(pool, _pool_ref(conv, 0))


@pytest.mark.parametrize("mode", [MODE_FP32, MODE_BF16])
@pytest.mark.parametrize("h,w", [(32, 32), (33, 47)])
def test_retina_stem_pool_is_the_maximum_of_its_window(engine_face, h, w, mode):
    """torchvision's MaxPool2d(3, 2, 1).  32 x 32 -> stem 16 x 16 -> 8 x 8: padded taps on the top and left edges only;
    33 x 47 -> 17 x 24 -> 9 x 12: the odd height puts one below the last row as well, two frames put a frame behind an edge."""
    frames = torch.from_numpy(synth.video_frames(901, 2, h, w))
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    mh, mw = (oh - 1) // 2 + 1, (ow - 1) // 2 + 1
    run = lambda: engine_face.face_forward(frames, mode)
    conv = _tap(run, engine_face, "face_stem_conv", (2, oh, ow, 64), mode)
    pool = _tap(run, engine_face, "face_pool", (2, mh, mw, 64), mode)
    assert conv.abs().max() > 0 and torch.equal(pool, _pool_ref(conv, 1))


@pytest.mark.parametrize("mode", [MODE_FP32, MODE_BF16, MODE_F16X3])
def test_static_forward_nchw_matches_the_u8_entry(engine_static, mode):
    """The preprocessed tensor of a frame (data/utils.py:19-39) through static_forward_nchw against the frame itself through
    static_forward: two writers of one image (in the x3 mode the fused u8 stem against the planar hi / lo image), probabilities
    within the 1e-4 that test_gpu_dropin.py holds the mirror of this entry point to."""
    frame = synth.face_frames(1234, 1)
    _, p_u8, _ = engine_static.static_forward(torch.from_numpy(frame), mode)
    _, p_x, _ = engine_static.static_forward_nchw(ov.pth_processing(frame), mode)
    d = (p_x - p_u8).abs().max().item()
    print("mode", mode, "max|dprob| nchw vs u8", d)
    assert d < 1e-4
