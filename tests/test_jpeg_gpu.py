"""GPU checks of data.jpeg.JpegDecoder / decode_jpeg_batch: the decoded images against the pixels Pillow returned for the same streams
(tests/golden/g16_jpeg.npz), bit for bit; the fallback routes; corrupt streams; the two alternating staging sets; and the decoded images as the input of
collate_train_raw and raw_plan_for."""
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from pytorch_object_detection_amd import _lib, ops  # noqa: E402
from pytorch_object_detection_amd._lib import FdError  # noqa: E402
from pytorch_object_detection_amd.data import JpegDecoder, collate_train_raw, decode_jpeg_batch  # noqa: E402
from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS  # noqa: E402
from test_model_gpu import randomize_norms  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G16 = os.path.join(HERE, "golden", "g16_jpeg.npz")


@pytest.fixture(scope="module")
def g16():
    g = np.load(G16)
    return {k: g[k] for k in g.files}


def _supported(g):
    n = len(g["params"])
    return [g[f"jpg_{i}"].tobytes() for i in range(n)], [g[f"rgb_{i}"] for i in range(n)]


def test_decode_equals_pillow_on_every_supported_case(g16):
    blobs, want = _supported(g16)
    whole = decode_jpeg_batch(blobs, DEV)                       # the whole supported set as ONE batch: 104 images, 260 component jobs
    assert len(whole) == len(blobs)
    for i, (t, w) in enumerate(zip(whole, want)):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == w.shape, i
        np.testing.assert_array_equal(t.cpu().numpy(), w, err_msg=f"case {i} {g16['params'][i].tolist()} in the whole batch")
    dec = JpegDecoder(DEV, threads=3, fallback="raise")
    for lo in range(0, len(blobs), 13):                         # and in batches of 13 (the last one shorter), bytes and uint8 arrays alike
        part = [b if k % 2 else np.frombuffer(b, np.uint8) for k, b in enumerate(blobs[lo:lo + 13])]
        for i, t in enumerate(dec.decode(part), lo):
            np.testing.assert_array_equal(t.cpu().numpy(), want[i], err_msg=f"case {i}")


def test_unsupported_streams_fall_back_to_pillow_or_raise(g16):
    blobs, want = _supported(g16)
    bad = [g16[f"bad_{k}"].tobytes() for k in range(len(g16["bad_reason"]))]
    strict = JpegDecoder(DEV, fallback="raise")
    for k, reason in enumerate(g16["bad_reason"]):
        with pytest.raises(FdError, match="stream 2 is not supported") as ei:
            strict.decode([blobs[3], blobs[4], bad[k]])
        assert ei.value.rc == _lib.E_UNSUPPORTED and _lib.JPEG_REASONS[int(reason)] in str(ei.value)
    pytest.importorskip("PIL")
    soft = JpegDecoder(DEV, fallback="pil")
    ks = [k for k in range(len(bad)) if f"bad_rgb_{k}" in g16]
    assert len(ks) >= 2
    mixed = [blobs[40]] + [bad[k] for k in ks] + [blobs[41]]
    got = soft.decode(mixed)
    np.testing.assert_array_equal(got[0].cpu().numpy(), want[40])
    np.testing.assert_array_equal(got[-1].cpu().numpy(), want[41])
    for k, t in zip(ks, got[1:-1]):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
        np.testing.assert_array_equal(t.cpu().numpy(), g16[f"bad_rgb_{k}"], err_msg=f"unsupported stream {k}")
    only = soft.decode([bad[ks[0]]])                            # a call with nothing for the HIP path
    np.testing.assert_array_equal(only[0].cpu().numpy(), g16[f"bad_rgb_{ks[0]}"])


def test_a_truncated_stream_raises_and_launches_nothing(g16):
    blobs, want = _supported(g16)
    dec = JpegDecoder(DEV)
    big = max(range(len(blobs)), key=lambda i: len(blobs[i]))
    info = ops.jpeg_parse(blobs[big])
    cut = blobs[big][:int(info.scan_offset) + (len(blobs[big]) - int(info.scan_offset)) // 2]        # the headers are whole, the scan is not
    first = dec.decode([blobs[7], blobs[8]])
    torch.cuda.synchronize()
    launches = ops.LAUNCHES[0]
    with pytest.raises(FdError, match="stream 1 is corrupt") as ei:
        dec.decode([blobs[9], cut, blobs[10]])
    assert ei.value.rc == _lib.JPEG_E_TRUNCATED
    with pytest.raises(FdError, match="stream 0 is corrupt"):
        dec.decode([blobs[9][:50]])
    assert ops.LAUNCHES[0] == launches                          # no C-ABI launch was enqueued for either call
    np.testing.assert_array_equal(first[0].cpu().numpy(), want[7])
    again = dec.decode([blobs[9], blobs[10]])                   # the decoder is usable afterwards
    np.testing.assert_array_equal(again[0].cpu().numpy(), want[9])
    np.testing.assert_array_equal(again[1].cpu().numpy(), want[10])


def test_consecutive_calls_do_not_corrupt_each_others_staging(g16):
    blobs, want = _supported(g16)
    dec = JpegDecoder(DEV, fallback="raise")
    a, b, c = list(range(0, 40)), list(range(60, 104)), list(range(30, 70))
    ra = dec.decode([blobs[i] for i in a])                      # nothing synchronises between the three calls: set 0, set 1, set 0 again
    rb = dec.decode([blobs[i] for i in b])
    rc = dec.decode([blobs[i] for i in c])
    for idx, res in ((a, ra), (b, rb), (c, rc)):
        for i, t in zip(idx, res):
            np.testing.assert_array_equal(t.cpu().numpy(), want[i], err_msg=f"case {i}")
    assert dec._sets[0].coef is not dec._sets[1].coef and dec._sets[0].coef.is_pinned() and dec._sets[1].tab.is_pinned()


def test_decoded_images_feed_collate_train_raw_and_raw_plans(g16):
    blobs, want = _supported(g16)
    p = g16["params"]
    pick = [i for i in range(len(p)) if (p[i, 1], p[i, 2]) in ((33, 47), (40, 48)) and p[i, 0] in (0, 2)]
    assert len(pick) == 4
    decoded = decode_jpeg_batch([blobs[i] for i in pick], DEV, fallback="raise")
    uploaded = [torch.from_numpy(want[i]).to(DEV) for i in pick]
    boxes = [np.array([[2., 3., 20., 25.], [10., 5., 40., 30.]], np.float32)] * 4
    classes = [np.array([1, 5])] * 4
    got = collate_train_raw(decoded, boxes, classes, (96, 160), rng=random.Random(3))
    exp = collate_train_raw(uploaded, boxes, classes, (96, 160), rng=random.Random(3))
    for u, v in zip(got, exp):
        assert torch.equal(u, v)
    torch.manual_seed(5)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).eval()
    randomize_norms(model, 7)
    model.to(DEV)
    plan = model.raw_plan_for(decoded, (96, 160))
    plan.run()
    out_dec = [[t.clone() for t in grp] for grp in model.outputs_of(plan)]
    plan = model.raw_plan_for(uploaded, (96, 160))
    plan.run()
    for ge, gg in zip(out_dec, model.outputs_of(plan)):
        for u, v in zip(ge, gg):
            assert torch.equal(u, v)
