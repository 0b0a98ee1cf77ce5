"""video_corpus.run_video_corpus: three face folders run in packed passes give, bit for bit, what preprocess_video_and_predict(decode=
"device") gives for each folder alone -- tables, present masks and CSV files --, for passes of 1, 5 and 1000 tiles and both entropy modes.

The corpus, written here with PIL.Image.save (synthetic models):
    seven   files 0..6 of 7 frames, 25 fps (LSTM step 5): windows at frames 0 and 5
    one     file 5 alone of 8 frames, 25 fps: zero rows in front of it, its rows held behind it
    gaps    files {0, 1, 5, 6, 11} of 12 frames, 30 fps (step 6): windows at 0 and 6, a reset in between, held and own rows mixed
Crop sizes run from 17 x 23 to 64 x 48; the files are 4:2:0 but for one 4:4:4 file, one grey file and one progressive file, which
the device path hands to PIL.  13 tiles: passes of 5 end inside `seven` and inside `gaps`."""
import os

import numpy as np
import pytest
import torch

from avcer_amd import jpeg
from avcer_amd.engine import MODE_F16X3, MODE_FP32
from avcer_amd.video_corpus import FaceFolder, run_video_corpus
from avcer_amd.video_pipeline import preprocess_video_and_predict, read_face_dir

pytestmark = pytest.mark.gpu

SIZES = [(17, 23), (64, 48), (33, 40), (48, 64), (23, 17), (40, 33), (64, 48), (31, 31), (50, 21), (17, 23), (64, 47), (19, 48), (37, 29)]  # (w, h)
SPEC = (("seven", range(7), 7, 25), ("one", [5], 8, 25), ("gaps", [0, 1, 5, 6, 11], 12, 30))
ENTROPY = ("host", "device")


def crop(seed, w, h):
    """A smooth picture with some texture: blocks of 8 random colours, blurred by repetition, plus a little noise."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2, 3)).astype(np.float32)
    img = np.kron(coarse, np.ones((8, 8, 1), dtype=np.float32))[:h, :w]
    return np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def eng(engine_static, engine_dynamic):
    return engine_dynamic


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    from PIL import Image

    root = tmp_path_factory.mktemp("faces")
    folders, k = [], 0
    for name, numbers, total, fps in SPEC:
        os.makedirs(root / name / "00")
        for i in numbers:
            w, h = SIZES[k]
            img, kw = Image.fromarray(crop(100 + k, w, h)), dict(quality=95)
            if k == 2:
                img = img.convert("L")                 # a grey file
            elif k == 4:
                kw["subsampling"] = 0                  # 4:4:4
            elif k == 9:
                kw["progressive"] = True               # not for the device path: PIL
            img.save(root / name / "00" / (str(i).zfill(6) + ".jpg"), "JPEG", **kw)
            k += 1
        folders.append(FaceFolder(name, str(root / name), fps, total))
    assert k == len(SIZES) == 13
    return folders


def files_of(path):
    out = {}
    for n in sorted(os.listdir(path)):
        with open(os.path.join(path, n), "rb") as f:
            out[n] = f.read()
    return out


@pytest.fixture(scope="module")
def alone(eng, corpus, tmp_path_factory):
    """Every folder on its own through the per-folder call, once per (mode, entropy; "pil": decode="pil"): {(mode, entropy): ([(stat,
    dyn)], CSV files)}, and the masks of read_face_dir.  Computed once, shared, left unchanged."""
    out = {}
    for mode, entropy in [(MODE_F16X3, e) for e in ENTROPY] + [(MODE_FP32, "host"), (MODE_F16X3, "pil")]:
        save = str(tmp_path_factory.mktemp(f"alone_{mode}_{entropy}"))
        tables = []
        for f in corpus:
            how = dict(decode="pil") if entropy == "pil" else dict(decode="device", jpeg_entropy=entropy)
            dyn, stat = preprocess_video_and_predict(eng, f.path, save, f.fps, f.total_frames, True, mode, **how)
            tables.append((torch.from_numpy(stat).to(eng.device), torch.from_numpy(dyn).to(eng.device)))
        out[mode, entropy] = (tables, files_of(save))
        assert len(out[mode, entropy][1]) == 6
    out["present"] = [read_face_dir(f.path, f.total_frames)[1] for f in corpus]
    return out


def assert_same(got, corpus, alone, mode, entropy, what=""):
    for f, g, (stat, dyn), present in zip(corpus, got, alone[mode, entropy][0], alone["present"]):
        assert g["name"] == f.name
        for key, want in (("static_probs", stat), ("dynamic_logits", dyn), ("present", torch.from_numpy(present).to(stat.device))):
            assert g[key].is_cuda and g[key].dtype == want.dtype and torch.equal(g[key], want), (what, f.name, key)


def test_the_corpus_crosses_both_sampling_paths_and_the_pil_fallback(eng, corpus):
    blobs = [open(os.path.join(f.path, "00", n), "rb").read() for f in corpus for n in sorted(os.listdir(os.path.join(f.path, "00")))]
    desc = [jpeg.probe(eng.lib, b) for b in blobs]
    assert sorted({(int(d["ncomp"]), int(d["hs"]), int(d["vs"])) for d in desc if d["status"] == jpeg.OK}) == [(1, 1, 1), (3, 1, 1), (3, 2, 2)]
    paths = jpeg.decode_tiles(eng, blobs)[1]
    assert paths.count("pil") == 1 and paths[9] == "pil"


@pytest.mark.parametrize("entropy", ENTROPY)
@pytest.mark.parametrize("per", [1, 5, 1000])
def test_same_bits_and_files_as_every_folder_alone(eng, corpus, alone, tmp_path, per, entropy):
    got = run_video_corpus(eng, corpus, MODE_F16X3, max_frames_per_pass=per, entropy=entropy, save_path=str(tmp_path), flag_save_prob=True)
    assert got.passes == {"static": {1: [1] * 13, 5: [5, 5, 3], 1000: [13]}[per], "lstm": [5]}
    assert_same(got, corpus, alone, MODE_F16X3, entropy, f"per={per} entropy={entropy}")
    assert [g["static_probs"].shape[0] for g in got] == [7, 8, 12]
    # the tables are not trivially alike: zero rows in front of `one`'s crop, a held row behind it, an LSTM output at its frame
    one = got[1]
    assert not one["static_probs"][:5].any() and one["static_probs"][5].any() and torch.equal(one["static_probs"][7], one["static_probs"][5])
    assert not one["dynamic_logits"][:5].any() and one["dynamic_logits"][5].any()
    assert files_of(tmp_path) == alone[MODE_F16X3, entropy][1]                     # the two CSV files per folder, byte for byte
    assert eng.x3_overflow_count(reset=False) == 0


def test_fp32_lstm_passes_and_pil_decode(eng, corpus, alone):
    got = run_video_corpus(eng, corpus, MODE_FP32, max_frames_per_pass=5, max_windows_per_pass=2)
    assert got.passes == {"static": [5, 5, 3], "lstm": [2, 2, 1]}
    assert_same(got, corpus, alone, MODE_FP32, "host", "fp32")
    assert not torch.equal(got[0]["static_probs"], alone[MODE_F16X3, "host"][0][0][0])  # the two modes' bits differ: both were compared
    # decode="pil" against the per-folder call's decode="pil": the tiles come from PIL's own resize there and here
    assert_same(run_video_corpus(eng, corpus, MODE_F16X3, max_frames_per_pass=5, decode="pil"), corpus, alone, MODE_F16X3, "pil", "pil")


def test_skip_failed_leaves_the_others_their_bits(eng, corpus, alone, tmp_path):
    os.makedirs(tmp_path / "bare" / "01")
    bare = FaceFolder("bare", str(tmp_path / "bare"), 25, 4)
    mixed = [corpus[0], bare] + corpus[1:]
    eng.profile_enable(True)
    try:
        eng.profile_read_launches()
        with pytest.raises(FileNotFoundError, match="folder bare: no track directory"):
            run_video_corpus(eng, mixed, MODE_F16X3, max_frames_per_pass=5)
        assert eng.profile_read_launches() == []                                   # refused before any launch
    finally:
        eng.profile_enable(False)
    got = run_video_corpus(eng, mixed, MODE_F16X3, max_frames_per_pass=5, skip_failed=True)
    assert [g["name"] for g in got] == ["seven", "bare", "one", "gaps"]
    assert set(got[1]) == {"name", "error"} and isinstance(got[1]["error"], FileNotFoundError) and "bare" in str(got[1]["error"])
    assert got.passes["static"] == [5, 5, 3]
    assert_same([got[0], got[2], got[3]], corpus, alone, MODE_F16X3, "host", "skip_failed")


def test_gemm_family_launches(eng, corpus, alone):
    """One folder costs what the per-folder call costs; three folders in one pass cost fewer launches than three per-folder calls --
    a count, not a time: 13 tiles share one static pass and 5 windows one LSTM call."""
    def launches(fn):
        torch.cuda.synchronize()
        eng.gemm_stats(reset=True)
        fn()
        torch.cuda.synchronize()
        return eng.gemm_stats(reset=True)[0]

    def loop(folders):
        for f in folders:
            preprocess_video_and_predict(eng, f.path, "", f.fps, f.total_frames, False, MODE_F16X3, decode="device")

    one_loop, one_packed = launches(lambda: loop(corpus[:1])), launches(lambda: run_video_corpus(eng, corpus[:1], MODE_F16X3))
    all_loop, all_packed = launches(lambda: loop(corpus)), launches(lambda: run_video_corpus(eng, corpus, MODE_F16X3))
    print(f"GEMM-family launches: one folder {one_loop} (loop) {one_packed} (packed); three folders {all_loop} (loop) {all_packed} (packed)")
    assert one_loop > 0 and one_packed == one_loop
    assert all_packed < all_loop


@pytest.mark.parametrize("entropy", ENTROPY)
def test_decode_tiles_into_a_slice_at_an_offset(eng, corpus, entropy):
    """decode_tiles(out=buffer[3:3 + n]): the same tiles as the plain call, and every byte of the buffer outside the slice keeps its
    guard value -- two runs with patterns that differ in every byte, as tests/guard_band.py fills them."""
    blobs = [open(os.path.join(f.path, "00", n), "rb").read() for f in corpus for n in sorted(os.listdir(os.path.join(f.path, "00")))]
    n = len(blobs)
    want, want_paths = jpeg.decode_tiles(eng, blobs, entropy=entropy)
    for pattern in (0xA5, 0x5A):
        buf = torch.full((n + 5, 224, 224, 3), pattern, dtype=torch.uint8, device=eng.device)
        tiles, paths = jpeg.decode_tiles(eng, blobs, entropy=entropy, out=buf[3:3 + n])
        torch.cuda.synchronize()
        assert tiles.data_ptr() == buf[3].data_ptr() and paths == want_paths
        assert torch.equal(buf[3:3 + n], want)
        assert bool((buf[:3] == pattern).all()) and bool((buf[3 + n:] == pattern).all())
    for bad in (torch.empty(n + 1, 224, 224, 3, dtype=torch.uint8, device=eng.device), torch.empty(n, 224, 224, 3, dtype=torch.uint8),
                torch.empty(n, 224, 224, 3, dtype=torch.int8, device=eng.device),
                torch.empty(n, 224, 448, 3, dtype=torch.uint8, device=eng.device)[:, :, ::2]):
        with pytest.raises(ValueError, match="decode_tiles: out must be"):
            jpeg.decode_tiles(eng, blobs, entropy=entropy, out=bad)
