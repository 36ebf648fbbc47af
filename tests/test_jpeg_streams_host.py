"""CPU checks of the baseline JPEG writer (tests/jpeg_writer.py) and of the corpus it writes
(tests/jpeg_stream_cases.py): Pillow opens every file, the parser sorts it as the expected route implies, and the
numpy model of test_jpeg_host.py reads back the very coefficients the writer was given and turns them into Pillow's
pixels.  Writer, model and Pillow are checked against each other here before test_jpeg_streams_gpu.py brings the
device in."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_stream_cases as C
import jpeg_writer as W
import test_jpeg_host as H
from on_device_image_captioning_amd import jpeg as J

# "host" by design, and nothing else: jpeg_stream_cases.py gives the reason for each
HOST_CASES = {"symbols_run_past_63", "symbols_dc_overflow", "layout_fill", "header_adobe0"}
# the model stops at an 0xFF 0xFF pair inside the scan (`_intervals`); the only such case is "host" anyway
MODEL_CANNOT_READ = {"layout_fill"}


def pil_rgb(blob):
    im = Image.open(io.BytesIO(blob))
    assert im.mode == "RGB"
    return np.asarray(im)


def test_the_corpus_covers_what_it_names():
    names = list(C.CASES)
    assert len(names) == len(set(names)) >= 90
    assert set(C.names(C.HOST)) == HOST_CASES
    for prefix in ("huff_", "symbols_", "restart_", "layout_", "header_", "size_", "sync_"):
        assert any(n.startswith(prefix) for n in names), prefix
    for n in HOST_CASES:
        rec = C.build(n)[2]
        assert rec["why_host"] and rec["host_by"] in ("parser", "status")
    assert MODEL_CANNOT_READ <= HOST_CASES


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_against_pillow_parser_and_model(name):
    """Building the case asserts its own precondition.  Then: Pillow yields an RGB image of the declared size; the
    parser gives the kind the route implies; for a device case the model reads back the writer's input coefficients
    and its pixels are Pillow's."""
    blob, route, rec = C.build(name)
    want = pil_rgb(blob)
    w, h = rec["size"]
    assert want.shape == (h, w, 3)
    hd = J.parse(blob)
    if route == C.HOST and rec["host_by"] == "parser":
        assert hd.kind == J.HOST and hd.reason
        return
    assert hd.kind == J.DEVICE, hd.reason                  # a "status" host case is the device's to turn away
    assert (hd.width, hd.height, hd.sampling) == (w, h, rec["sampling"])
    if route == C.HOST:
        return
    coefs = H.model_coefficients(blob, hd)
    assert coefs.shape == rec["coefs"].shape and np.array_equal(coefs, rec["coefs"])
    got = H.model_rgb(blob)                                # raises Rejected outside the device's IDCT range
    assert np.array_equal(got, want), int(np.abs(got.astype(int) - want).max())


def test_host_by_status_cases_fail_in_the_model_for_their_stated_reason():
    blob, _, _ = C.build("symbols_dc_overflow")
    hd = J.parse(blob)
    with pytest.raises(H.Rejected, match="DC"):
        H.model_dc_prediction(H.model_coefficients(blob, hd), hd)
    blob, _, _ = C.build("symbols_run_past_63")
    with pytest.raises(IndexError):                        # zig-zag index 64
        H.model_coefficients(blob, J.parse(blob))
    blob, _, rec = C.build("layout_fill")
    with pytest.raises(AssertionError, match="marker FF"):
        H.model_coefficients(blob, J.parse(blob))
    plain = C.build("layout_tile_boundaries")[0]
    assert np.array_equal(pil_rgb(blob), pil_rgb(plain))   # Pillow reads through the fill bytes


def test_symbol_0x50_ends_the_block_for_libjpeg_and_the_model():
    """Nothing of a block is read behind a 0x50: the blocks that hold one keep only what stood in front of it."""
    blob, route, rec = C.build("symbols_0x50")
    assert route == C.DEVICE
    hd = J.parse(blob)
    coefs = H.model_coefficients(blob, hd)
    assert np.count_nonzero(coefs[3 * 3]) == 2 and np.count_nonzero(coefs[7 * 3 + 1]) == 0   # Y block 3, Cb block 7
    assert np.array_equal(coefs, rec["coefs"])


def test_the_record_describes_the_bytes():
    for name in ("layout_tile_boundaries", "restart_1_289_444", "huff_fffe_h2v2", "layout_zero_pad_bits"):
        blob, _, rec = C.build(name)
        scan = blob[rec["blob_scan_offset"]:]
        assert J.parse(blob).data_offset == rec["blob_scan_offset"]
        assert scan[rec["scan_len"]:rec["scan_len"] + 2] == b"\xff\xd9"
        body = np.frombuffer(scan[:rec["scan_len"] + 1], np.uint8)
        ff = np.flatnonzero(body[:-1] == 0xFF)
        assert sorted(rec["ff00"] + rec["rst"]) == ff.tolist()
        assert all(body[i + 1] == 0 for i in rec["ff00"])
        assert [int(body[i + 1]) for i in rec["rst"]] == [0xD0 + k % 8 for k in range(len(rec["rst"]))]
        emitted = sum(sum(v.values()) for v in rec["lengths"].values())
        assert emitted == sum(sum(v.values()) for v in rec["symbols"].values()) > 0


# ------------------------------------------------------------------------------------------------------------
# the writer's own rules
# ------------------------------------------------------------------------------------------------------------
def test_writer_refuses_an_overfull_huffman_table():
    full = ([2] + [0] * 15, bytes([0, 1]))                 # codes 0 and 1: the all-ones code of length 1
    with pytest.raises(ValueError, match="overflows"):
        W.check_table(full)
    with pytest.raises(ValueError, match="overflows"):
        W.table_with_lengths([(s, 8) for s in range(256)])               # 256 codes of 8 bits
    with pytest.raises(ValueError, match="overflows"):
        W.table_with_lengths([(s, s + 1) for s in range(16)] + [(16, 16)])   # one past 0xFFFE
    W.table_with_lengths([(s, s + 1) for s in range(16)])                # 0xFFFE itself is legal
    coefs = [np.zeros((1, 64), np.int64)] * 3
    with pytest.raises(ValueError, match="overflows"):
        W.write_jpeg(8, 8, 0, coefs, C.Q3, dc_tables=[full] * 3, layout=W.Layout(dc_ids=(0, 0, 0)))
    assert J.parse(W.write_jpeg(8, 8, 0, coefs, C.Q3)[0]).kind == J.DEVICE
    # the parser refuses the same tables
    good = W.write_jpeg(8, 8, 0, coefs, C.Q3, dc_tables=[([1] + [0] * 15, b"\x00")] * 3,
                        layout=W.Layout(dc_ids=(0, 0, 0)))[0]
    assert J.parse(good).kind == J.DEVICE
    i = good.index(b"\xff\xc4") + 5
    assert good[i] == 1
    assert J.parse(good[:i] + b"\x02" + good[i + 1:]).reason in ("bad Huffman table", "bad DHT length")
    with pytest.raises(ValueError):
        W.write_jpeg(8, 8, 0, coefs, C.Q3, raw_blocks={(0, 0): [(0, None), (0x50, None)]})   # no code for 0x50


def test_tables_from_frequencies_respect_the_length_limit():
    fib = {0: 1, 1: 1}
    for s in range(2, 40):
        fib[s] = fib[s - 1] + fib[s - 2]                   # unlimited Huffman would need codes of up to 39 bits
    for limit in (16, 12):
        bits, vals = W.table_from_frequencies(fib, max_len=limit)
        assert sorted(vals) == list(range(40)) and sum(bits) == 40 and not any(bits[limit:])
        codes = W.table_codes((bits, vals))
        assert codes[39][1] < codes[0][1]                  # the likelier symbol has the shorter code
        assert all(code != (1 << length) - 1 for code, length in codes.values())     # all-ones stays free
    uniform = W.table_from_frequencies({s: 5 for s in range(256)})
    assert len(uniform[1]) == 256 and max(n for n in range(16) if uniform[0][n]) + 1 == 9


def test_block_symbols_and_back():
    rng = np.random.default_rng(3)
    for _ in range(50):
        block = rng.integers(-1023, 1024, 64) * (rng.random(64) < rng.random())
        block[0] = rng.integers(-2047, 2048)
        syms = W.block_symbols(block)
        assert np.array_equal(W.symbols_block(syms), block)
        assert (syms[-1][0] == W.EOB) == (block[63] == 0)
        assert all(s == W.ZRL or s == W.EOB or s in W.REGULAR_AC for s, _ in syms[1:])
    assert W.amplitude_bits(-3, 2) == 0 and W.amplitude_bits(3, 2) == 3 and W.amplitude_bits(-1023, 10) == 0


@pytest.mark.parametrize("sampling", [0, 1, 2], ids=C.SAMPLING_NAMES)
@pytest.mark.parametrize("restart", [0, 3])
def test_plain_files_parse_like_a_pillow_save(sampling, restart):
    """Standard tables, JFIF, one segment per table: the header fields are those of a Pillow save with the same
    quantisation tables, sampling and restart interval."""
    size = (43, 29)
    img = H.smooth_rgb(size[1], size[0], seed=1)
    qt = [C.COARSE, C.FINE, C.FINE]
    ref = J.parse(H.encode(img, qtables=[[int(v) for v in q] for q in qt[:2]], subsampling=sampling,
                           restart_marker_blocks=restart))
    coefs = W.coefficients_from_pixels(img, sampling, qt, restart)
    mine = J.parse(W.write_jpeg(*size, sampling, coefs, qt, restart=restart)[0])
    assert ref.kind == mine.kind == J.DEVICE
    assert H.header_fields(mine) == H.header_fields(ref)
