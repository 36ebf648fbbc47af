"""The corpus of tests/jpeg_prog_stream_cases.py (progressive scan scripts no Pillow save produces) through the device
JPEG decoder with progressive="device", against Pillow bit for bit: each file alone, the whole corpus as one batch in
two orders beside baseline files, the device cases with the PIL fallback taken away, the host-by-design cases, the
coefficients left in the workspace against the writer's input, and the scaled decode."""
import io
import random
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_prog_stream_cases as C
import jpeg_stream_cases as B
import test_jpeg_host as H
from on_device_image_captioning_amd import jpeg as J
from test_jpeg_draft_gpu import decode_and_compare
from test_jpeg_draft_host import model_draft_rgb, request_for

pytestmark = pytest.mark.gpu

N_HOST = 7                                                 # "host" by design: jpeg_prog_stream_cases.py lists them
HOST_ROUTES = {"parser": "host", "status": "host-after-status"}
BASELINE = ("huff_shared_444", "restart_short_last_h2v2")  # two files of the baseline corpus for the mixed batches


@pytest.fixture(scope="module")
def pre():
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    return DevicePreprocessor(384, "cuda:0")


@pytest.fixture(scope="module")
def corpus():
    return {name: C.build(name) for name in C.CASES}


@pytest.fixture(scope="module")
def pillow(corpus):
    """Pillow's pixels of every file of the corpus and of the two baseline files: computed once, never changed."""
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, blob in [(n, v[0]) for n, v in corpus.items()] + [(n, B.build(n)[0]) for n in BASELINE]:
            a = np.asarray(Image.open(io.BytesIO(blob)))
            a.setflags(write=False)
            out[blob] = a
    return out


def want_route(route, rec):
    return "device-progressive" if route == C.DEVICE else HOST_ROUTES[rec["host_by"]]


def check(pre, pillow, blobs, routes):
    got = pre.decode_jpeg(blobs, progressive="device")
    assert len(got) == len(blobs) == len(pre.last_routes)
    for k, (g, b) in enumerate(zip(got, blobs)):
        assert pre.last_routes[k] == routes[k], (k, pre.last_routes[k], routes[k])
        g = g.cpu().numpy()
        assert g.shape == pillow[b].shape, (k, g.shape)
        assert np.array_equal(g, pillow[b]), (k, int(np.abs(g.astype(int) - pillow[b]).max()))
    return got


def test_each_case_alone(pre, corpus, pillow):
    """Every file in a call of its own: Pillow's pixels, by the route the case names.  All cases are tried; the
    failures are reported together."""
    bad = []
    for name, (blob, route, rec) in corpus.items():
        try:
            check(pre, pillow, [blob], [want_route(route, rec)])
        except AssertionError as e:
            bad.append((name, str(e)[:80]))
    assert not bad, bad


def test_whole_corpus_as_one_batch_in_two_orders(pre, corpus, pillow):
    files = {n: (v[0], want_route(v[1], v[2])) for n, v in corpus.items()}
    files.update({n: (B.build(n)[0], "device") for n in BASELINE})
    runs = []
    for seed in (7, 8):
        order = list(files)
        random.Random(seed).shuffle(order)
        got = check(pre, pillow, [files[n][0] for n in order], [files[n][1] for n in order])
        runs.append({n: t.cpu() for n, t in zip(order, got)})
    assert all(torch.equal(runs[0][n], runs[1][n]) for n in files)


def test_device_cases_never_ask_pillow(pre, corpus, pillow, monkeypatch):
    """No silent host fallback: with the PIL decode taken away every device case still decodes."""
    def boom(blob, draft=None):
        raise AssertionError("host decode")
    monkeypatch.setattr(pre, "_host_rgb", boom)
    blobs = [blob for blob, route, _ in corpus.values() if route == C.DEVICE]
    assert len(blobs) == len(corpus) - N_HOST
    check(pre, pillow, blobs, ["device-progressive"] * len(blobs))
    check(pre, pillow, blobs[::-1], ["device-progressive"] * len(blobs))


def test_host_cases_come_back_as_pillow_decodes_them(pre, corpus, pillow):
    hosts = {n: v for n, v in corpus.items() if v[1] == C.HOST}
    assert len(hosts) == N_HOST
    for name, (blob, _, rec) in hosts.items():
        try:
            check(pre, pillow, [blob], [HOST_ROUTES[rec["host_by"]]])            # does not raise
        except AssertionError as e:
            raise AssertionError((name, rec["why_host"], str(e))) from None
    plain = corpus["std_h2v2"][0]                             # a host case does not disturb its neighbours
    blobs = [plain] + [v[0] for v in hosts.values()] + [plain]
    check(pre, pillow, blobs, ["device-progressive"] + [HOST_ROUTES[v[2]["host_by"]] for v in hosts.values()] +
          ["device-progressive"])


def test_coefficients_equal_the_writers_input(pre, corpus, pillow):
    """The entropy stage alone: what the four scan procedures leave in the workspace is what the writer was given, for
    every device case in one batch (the one large frame is decoded in the tests above)."""
    cases = [n for n, v in corpus.items() if v[1] == C.DEVICE and n not in C.BIG]
    assert len(cases) == len(corpus) - N_HOST - len(C.BIG)
    check(pre, pillow, [corpus[n][0] for n in cases], ["device-progressive"] * len(cases))
    bad = []
    for k, n in enumerate(cases):
        want = corpus[n][2]["coefs"]
        got = pre.progressive_coefficients(k).cpu().numpy()
        if got.shape != want.shape or not np.array_equal(got, want):
            where = np.argwhere(got != want)[:3].tolist() if got.shape == want.shape else got.shape
            bad.append((n, where))
    assert not bad, bad


@pytest.mark.parametrize("s", [2, 8])
def test_scaled_decode_of_the_corpus(pre, corpus, s):
    """Every case at scale 1 / s against Pillow's draft mode, with test_jpeg_draft_gpu.py's comparison and the admission
    rule of test_jpeg_streams_gpu.test_scaled_decode_of_the_corpus: an image too small for s is drafted at the scale
    Pillow picks instead, and a device case stays on the device wherever the model of the reduced transforms keeps it
    inside the range limits."""
    bad = []
    for name, (blob, route, rec) in corpus.items():
        size = rec["size"]
        try:
            req = request_for(size, s)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                routes, scales = decode_and_compare(pre, [blob], req, progressive="device")
            assert scales == [J.draft_scale(size, req)] and (scales == [s] or min(size) < 2 * s), scales
            if route != C.DEVICE:
                assert routes == (HOST_ROUTES[rec["host_by"]],), routes
                continue
            hd = J.parse_progressive(blob)
            try:
                if scales[0] > 1:
                    model_draft_rgb(None, scales[0], (hd, rec["coefs"].astype(np.int16)))
                assert routes == ("device-progressive",), routes
            except H.Rejected:
                assert routes == ("host-after-status",), routes
        except AssertionError as e:
            bad.append((name, str(e)[:80]))
    assert not bad, bad
