"""The result video on the GPU: avcer_annotate_frames against annotate.draw_numpy with tolerance zero (inside guard bands, at
odd frame addresses, under heavy overlap), annotate.write_result_video against PIL's drawing and PIL's JPEG files, and
run.run_inference_file(path_save_video=...)."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import guard_band as gb
from annotate_pil import draw_pil, overlap_orders, random_items, small_case
from avcer_amd import annotate as an
from avcer_amd import avi
from avcer_amd import run as arun
from avcer_amd.engine import MODE_F16X3
from avcer_amd.fusion import MODEL_ORDER
from test_avi_cpu import pcm_of, picture
from test_gpu_avi import KEYS, recording

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine_all(engine, sd_static, sd_dynamic, sd_audio):
    engine.load_static(sd_static)
    engine.load_dynamic(sd_dynamic)
    engine.load_audio(sd_audio)
    return engine


def test_kernel_equals_draw_numpy_inside_guard_bands(engine):
    """[3,37,53,3]: a frame is 5883 bytes, so frames 1 and 2 start at odd addresses; items cross every edge and lie outside."""
    frames, items, masks = small_case()
    want = an.draw_numpy(frames.copy(), items, masks)
    src = torch.from_numpy(frames).to(engine.device)
    flat, table = an.pack_masks(masks)
    flat_d = torch.from_numpy(flat).to(engine.device)

    def run(outs):
        outs[0].copy_(src)
        assert an.draw(engine, outs[0], items, (flat_d, table)) is outs[0]

    got, = gb.check(run, [gb.Band("frames", tuple(frames.shape), torch.uint8, row_bytes=3 * frames.shape[2])], inputs=(src, flat_d),
                    device=engine.device)
    np.testing.assert_array_equal(got.numpy(), want)
    np.testing.assert_array_equal(got.numpy()[1], frames[1])              # the frame without items
    # every byte offset of the batch in its allocation
    size = frames.size
    for off in (1, 2, 3, 5):
        buf = torch.full((64 + size + 64,), 0xA5, dtype=torch.uint8, device=engine.device)
        out = buf[off:off + size].view(frames.shape)
        out.copy_(src)
        an.draw(engine, out, items, masks)
        host = buf.cpu().numpy()
        assert (host[:off] == 0xA5).all() and (host[off + size:] == 0xA5).all(), off
        np.testing.assert_array_equal(host[off:off + size].reshape(frames.shape), want, err_msg=str(off))


def test_empty_lists_leave_the_frames_untouched_and_runs_agree(engine):
    frames, items, masks = small_case(2)
    a = torch.from_numpy(frames).to(engine.device)
    assert an.draw(engine, a, [], masks) is a and an.draw(engine, a, np.zeros(0, dtype=an.ITEM)) is a
    off_frame = [an.outline(0, (-30, -30, -10, -10), (1, 2, 3), 2), an.mask(2, (53, 0), (1, 2, 3), 0, 2)]
    an.draw(engine, a, off_frame, masks)
    np.testing.assert_array_equal(a.cpu().numpy(), frames)
    b = a.clone()
    an.draw(engine, a, items, masks)
    an.draw(engine, b, items, masks)
    assert torch.equal(a, b) and not torch.equal(a.cpu(), torch.from_numpy(frames))
    fr, masks1, order_a, order_b = overlap_orders()
    ga = an.draw(engine, torch.from_numpy(fr).to(engine.device), order_a, masks1).cpu().numpy()
    gb_ = an.draw(engine, torch.from_numpy(fr).to(engine.device), order_b, masks1).cpu().numpy()
    np.testing.assert_array_equal(ga, an.draw_numpy(fr.copy(), order_a, masks1))
    np.testing.assert_array_equal(gb_, an.draw_numpy(fr.copy(), order_b, masks1))
    assert (ga != gb_).any()


def test_refusals_come_before_the_launch(engine):
    frames, _, masks = small_case()
    a = torch.from_numpy(frames).to(engine.device)
    good = an.outline(1, (1, 1, 5, 5), (1, 2, 3), 1)
    for bad, match in ((an.outline(3, (1, 1, 5, 5), (1, 2, 3), 1), r"item 1 \(OUTLINE\): frame 3"),
                       (an.fill(2, (1, 1, 5, 5), (1, 2, 3), 0), r"item 1 \(FILL\): coverage 0"),
                       (an.mask(2, (1, 1), (1, 2, 3), 2, 1), r"item 1 \(MASK\): mask index 2"),
                       (an.mask(2, (1, 1), (1, 2, 3), 0, 0), r"item 1 \(MASK\): scale 0")):
        with pytest.raises(ValueError, match=match):
            an.draw(engine, a, [good, bad], masks)
    with pytest.raises(ValueError, match="frames"):
        an.draw(engine, torch.from_numpy(frames), [good], masks)
    np.testing.assert_array_equal(a.cpu().numpy(), frames)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_order_holds_under_heavy_overlap(engine, seed):
    """200 random items per frame on [2,128,192,3]: every pixel lies under many items, and the picture is the sequential one."""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (2, 128, 192, 3), dtype=np.uint8)
    masks = [rng.integers(0, 256, (int(rng.integers(3, 20)), int(rng.integers(3, 30))), dtype=np.uint8) for _ in range(5)]
    items = random_items(rng, 2, 128, 192, 200, len(masks))
    want = an.draw_numpy(frames.copy(), items, masks)
    got = an.draw(engine, torch.from_numpy(frames).to(engine.device), items, masks).cpu().numpy()
    np.testing.assert_array_equal(got, want)


# ---------------------------------------------------------------------------------------------------- the file
def pil_file(bgr_frame, quality, subsampling):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr_frame[..., ::-1])).save(buf, "JPEG", quality=quality, subsampling=subsampling)
    return buf.getvalue()


def oracle_files(frames_bgr, records, pred, prob, quality, subsampling, panel=False):
    h, w = frames_bgr.shape[1:3]
    items, masks = an.layout(records, pred, prob, h, w, panel=panel)
    drawn = draw_pil(frames_bgr, items, masks)          # colours are symmetric or given in the frame's order: PIL draws the BGR array
    return [pil_file(f, quality, subsampling) for f in drawn]


@pytest.mark.parametrize("entropy", ["host", "device"])
def test_write_result_video_equals_pil_drawing_and_pil_files(engine, tmp_path, entropy):
    w, h, n = 96, 64, 5
    frames = np.stack([picture(w, h, 40 + i) for i in range(n)])
    records = np.array([[t, 0, 20 + t, 24, 70 + t, 60] for t in range(n)] + [[1, 1, 2, 2, 18, 20], [3, 1, 80, 30, 99, 70]], dtype=np.int64)
    prob = np.random.default_rng(8).dirichlet(np.ones(7), size=n)
    pred = prob.argmax(axis=1)
    pcm = pcm_of(9000, 2, seed=11)
    dev = torch.from_numpy(frames).to(engine.device)
    path = an.write_result_video(engine, dev, records, pred, prob, tmp_path / "out.avi", 30000, 1001, pcm=pcm, audio_rate=44100, quality=90,
                                 subsampling=2, entropy=entropy, frames_per_pass=2, panel=(entropy == "host"))
    np.testing.assert_array_equal(dev.cpu().numpy(), frames)               # the caller's frames are not drawn into
    want = oracle_files(frames, records, pred, prob, 90, 2, panel=(entropy == "host"))
    with avi.open_avi(path) as f:
        assert (f.n_frames, f.rate, f.scale, f.width, f.height, f.audio_rate, f.audio_channels) == (n, 30000, 1001, w, h, 44100, 2)
        np.testing.assert_array_equal(f.pcm, pcm)
        for i in range(n):
            assert bytes(f.frames[i]) == want[i], i
    assert want[0] != pil_file(frames[0], 90, 2)                            # and something was drawn


def test_run_inference_file_writes_the_result_video(engine_all, tmp_path):
    pcm = pcm_of(44100, 2, seed=5)
    path, blobs, dets = recording(tmp_path, "talk", 64, 48, 12, 30000, 1001, pcm, 400)
    with pytest.raises(ValueError, match="video_model"):
        arun.run_inference_file(engine_all, path, detections=dets, path_save_video=str(tmp_path / "no.avi"), video_model="AV+")
    assert not (tmp_path / "no.avi").exists()
    ref = arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_F16X3)
    assert "result_video" not in ref
    for model in ("av", "vd"):
        out_path = str(tmp_path / f"result_{model}.avi")
        got = arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_F16X3, path_save_video=out_path, video_model=model)
        assert got["result_video"] == out_path and set(got) == set(ref) | {"result_video"}
        for key in KEYS:
            np.testing.assert_array_equal(got[key], ref[key], err_msg=key)
        frames = np.stack([np.array(Image.open(io.BytesIO(b)).convert("RGB"))[..., ::-1] for b in blobs])
        k = [m.lower() for m in MODEL_ORDER].index(model)
        want = oracle_files(frames, got["records"], got[model], got["compound_prob"][k], 90, 2)
        with avi.open_avi(out_path) as f:
            assert (f.n_frames, f.rate, f.scale, f.audio_rate) == (12, 30000, 1001, 44100)
            np.testing.assert_array_equal(f.pcm, pcm)
            for i in range(12):
                assert bytes(f.frames[i]) == want[i], (model, i)
