"""The corpus of tests/jpeg_stream_cases.py (baseline streams no Pillow save produces) through the device JPEG decoder,
against Pillow bit for bit: each file alone under every knob set, the whole corpus as one batch in two orders, the
device cases with the PIL fallback taken away, the host-by-design cases, and the scaled decode."""
import random

import numpy as np
import pytest
import torch

import jpeg_stream_cases as C
import test_jpeg_host as H
from on_device_image_captioning_amd import jpeg as J
from test_jpeg_draft_gpu import decode_and_compare
from test_jpeg_draft_host import model_draft_rgb, request_for
from test_jpeg_gpu import KNOBS, check, pil_rgb

pytestmark = pytest.mark.gpu

KNOB_SETS = KNOBS + [dict(subseq_bits=4096)]              # 4096: kMaxSubseqBits of csrc/jpeg_decode.hip
KNOB_IDS = ["default", "serial", "subseq64", "subseq4096"]
HOST_ROUTES = {"parser": "host", "status": "host-after-status"}


@pytest.fixture(scope="module")
def pre():
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    return DevicePreprocessor(384, "cuda:0")


@pytest.fixture(scope="module")
def corpus():
    return {name: C.build(name) for name in C.CASES}


def want_route(route, rec):
    return "device" if route == C.DEVICE else HOST_ROUTES[rec["host_by"]]


@pytest.mark.parametrize("knobs", KNOB_SETS, ids=KNOB_IDS)
def test_each_case_alone(pre, corpus, knobs):
    """Every file in a call of its own: Pillow's pixels, by the route the case names.  All cases are tried; the
    failures are reported together."""
    bad = []
    for name, (blob, route, rec) in corpus.items():
        try:
            check(pre, [blob], **knobs)
            assert pre.last_routes == (want_route(route, rec),), pre.last_routes
        except AssertionError as e:
            bad.append((name, str(e)[:80]))
    assert not bad, bad


@pytest.mark.parametrize("knobs", KNOB_SETS, ids=KNOB_IDS)
def test_whole_corpus_as_one_batch_in_two_orders(pre, corpus, knobs):
    names = list(corpus)
    runs = []
    for seed in (7, 8):
        order = list(names)
        random.Random(seed).shuffle(order)
        check(pre, [corpus[n][0] for n in order], **knobs)
        assert pre.last_routes == tuple(want_route(*corpus[n][1:]) for n in order)
        got = pre.decode_jpeg([corpus[n][0] for n in order], **knobs)
        runs.append({n: t.cpu() for n, t in zip(order, got)})
    assert all(torch.equal(runs[0][n], runs[1][n]) for n in names)


def test_device_cases_never_ask_pillow(pre, corpus, monkeypatch):
    """No silent host fallback, as test_jpeg_gpu.test_every_image_is_decoded_on_the_device: with the PIL decode taken
    away every device case still decodes."""
    def boom(blob, draft=None):
        raise AssertionError("host decode")
    monkeypatch.setattr(pre, "_host_rgb", boom)
    blobs = [blob for blob, route, _ in corpus.values() if route == C.DEVICE]
    assert len(blobs) == len(corpus) - 4
    check(pre, blobs)
    assert set(pre.last_routes) == {"device"}
    check(pre, blobs[::-1], max_sync_passes=0)
    assert set(pre.last_routes) == {"device"}


def test_host_cases_come_back_as_pillow_decodes_them(pre, corpus):
    hosts = {n: v for n, v in corpus.items() if v[1] == C.HOST}
    assert len(hosts) == 4
    for name, (blob, _, rec) in hosts.items():
        for knobs in KNOB_SETS:
            got = pre.decode_jpeg([blob], **knobs)            # does not raise
            assert pre.last_routes == (HOST_ROUTES[rec["host_by"]],), (name, rec["why_host"])
            assert np.array_equal(got[0].cpu().numpy(), pil_rgb(blob)), name
    plain = corpus["huff_shared_444"][0]                      # a host case does not disturb its neighbours
    check(pre, [plain] + [v[0] for v in hosts.values()] + [plain])


def test_periodic_stream_that_never_synchronises(pre, corpus):
    """sync_periodic (see its docstring) with 64-bit units and the fewest sync passes the wrapper accepts above 0: the
    one interval cannot converge in one pass, so jpeg_serial_kernel has to walk it, stepping over the units whose
    recorded start state is exact (one in nine starts in phase, and unit 1 was redone from unit 0's exact end) and
    decoding the others again, which is the mixed branch of its loop.  DevicePreprocessor gives no view of which kernel
    ran, so the check is the pixels, under this and the neighbouring settings, alone and beside other files."""
    blob = corpus["sync_periodic"][0]
    other = corpus["restart_short_last_h2v2"][0]
    for passes in (1, 2, 3, 9):
        for bits in (64, 96, 160):
            check(pre, [blob], subseq_bits=bits, max_sync_passes=passes)
            assert pre.last_routes == ("device",)
    check(pre, [other, blob, other, blob], subseq_bits=64, max_sync_passes=1)
    assert pre.last_routes == ("device",) * 4


@pytest.mark.parametrize("s", [2, 8])
def test_scaled_decode_of_the_corpus(pre, corpus, s):
    """Every case at scale 1 / s against Pillow's draft mode, with test_jpeg_draft_gpu.py's comparison and its
    admission rule: an image too small for s is drafted at the scale Pillow picks instead, and a device case stays on
    the device wherever the model of the reduced transforms keeps it inside the range limits."""
    bad = []
    for name, (blob, route, rec) in corpus.items():
        size = rec["size"]
        try:
            req = request_for(size, s)
            routes, scales = decode_and_compare(pre, [blob], req)      # scales: what Pillow chose
            assert scales == [J.draft_scale(size, req)] and (scales == [s] or min(size) < 2 * s), scales
            if route != C.DEVICE:
                assert routes == (HOST_ROUTES[rec["host_by"]],), routes
                continue
            hd = J.parse(blob)
            try:
                if scales[0] > 1:
                    model_draft_rgb(None, scales[0], (hd, H.model_dc_prediction(rec["coefs"], hd)))
                assert routes == ("device",), routes
            except H.Rejected:
                assert routes == ("host-after-status",), routes
        except AssertionError as e:
            bad.append((name, str(e)[:80]))
    assert not bad, bad
