"""CPU side of one device decode batch: `jpeg.plan_device_batch` lays out the staging buffer that is uploaded in one
copy (record sections, scales, the files) and the RGB output.  Every offset the kernels follow comes from here, so the
layout is checked on the host: alignment, disjointness, the files' bytes, and that each record points into its own
file."""
import numpy as np
import pytest

from on_device_image_captioning_amd import jpeg as J
from test_jpeg_host import encode, smooth_rgb
from test_jpeg_progressive_host import encode_progressive

BASE = [encode(smooth_rgb(16, 16, seed=1), quality=90, subsampling=0),           # 16 x 16, 4:4:4
        encode(smooth_rgb(8, 24, seed=2), quality=90, subsampling=2)]            # 24 x 8, 4:2:0
PROG = [encode_progressive(smooth_rgb(16, 16, seed=3), quality=90, subsampling=0)]

#: (baseline files, progressive files, scales — baseline first)
CASES = {
    "mixed": (BASE, PROG, [1, 1, 1]),
    "mixed, one of each kind at 1/2": (BASE, PROG, [2, 1, 2]),
    "baseline only": (BASE, [], [1, 1]),
    "baseline only, one at 1/2": (BASE, [], [1, 2]),
    "progressive only": ([], PROG, [1]),
    "progressive only, at 1/2": ([], PROG, [2]),
}


def plan_of(blobs, pblobs, scales):
    hdrs, phdrs = [J.parse(b) for b in blobs], [J.parse_progressive(b) for b in pblobs]
    assert all(h.kind == J.DEVICE for h in hdrs + phdrs)
    assert all(not isinstance(h, J.ProgHeader) for h in hdrs) and all(h.scans for h in phdrs)
    return hdrs, phdrs, J.plan_device_batch([("base", hdrs, blobs), ("prog", phdrs, pblobs)], 2048, scales)


def test_the_test_files_are_what_they_should_be():
    hdrs, phdrs, _ = plan_of(*CASES["mixed"])
    assert [(h.width, h.height, h.sampling) for h in hdrs] == [(16, 16, 0), (24, 8, 2)]
    assert [(h.width, h.height) for h in phdrs] == [(16, 16)]


@pytest.mark.parametrize("case", CASES)
def test_staging_layout(case):
    blobs, pblobs, scales = CASES[case]
    hdrs, phdrs, p = plan_of(blobs, pblobs, scales)
    nb, npg = len(hdrs), len(phdrs)

    # sections: which ones there are, in the documented order, 256-aligned and disjoint from each other and the data
    kinds = [a.dtype for _, a in p.sections]
    want = ([J.HEADER_DTYPE] if nb else []) + ([J.PROG_HEADER_DTYPE, J.SCAN_DTYPE, J.TABLE_DTYPE] if npg else []) \
        + ([np.dtype(np.int32)] if max(scales) > 1 else [])
    assert kinds == want
    assert (p.tot is None) == (nb == 0) and (p.ptot is None) == (p.prog_off is None) == (npg == 0)
    assert (p.scale_off is None) == all(s == 1 for s in scales)
    spans = [(o, o + a.nbytes) for o, a in p.sections] + [(p.data_off, p.total)]
    assert all(lo % 256 == 0 for lo, _ in spans)
    assert spans == sorted(spans) and spans[0][0] == 0
    assert all(a_hi <= b_lo for (_, a_hi), (b_lo, _) in zip(spans, spans[1:])) and spans[-1][1] == p.total
    if npg:
        assert list(p.prog_off) == [o for o, a in p.sections if a.dtype in want[nb > 0:][:3]]
    if p.scale_off is not None:
        o, a = p.sections[-1]
        assert o == p.scale_off and list(a) == [s.bit_length() - 1 for s in scales]

    # the files: verbatim, back to back from data_off, baseline first, ending at `total`
    host = np.full(p.total + 64, 0xA5, np.uint8)
    p.fill(host)
    assert (host[p.total:] == 0xA5).all()
    pos = p.data_off
    assert len(p.blobs) == nb + npg
    for (o, a), blob in zip(p.blobs, blobs + pblobs):
        assert o == pos and host[o:o + len(blob)].tobytes() == blob and a.tobytes() == blob
        pos += len(blob)
    assert pos == p.total
    for o, a in p.sections:
        assert host[o:o + a.nbytes].tobytes() == a.tobytes()

    # records read back from the staging bytes, as the device reads them
    if nb:
        rec = host[:nb * J.HEADER_DTYPE.itemsize].view(J.HEADER_DTYPE)
        for r, h, (o, _), blob in zip(rec, hdrs, p.blobs, blobs):
            lo, hi = p.data_off + int(r["data_off"]), p.data_off + int(r["data_end"])
            assert (lo, hi) == (o + h.data_offset, o + len(blob))
            assert host[lo:hi].tobytes() == blob[h.data_offset:]
    if npg:
        n_scans = sum(len(h.scans) for h in phdrs)
        assert p.ptot["n_scans"] == n_scans
        srec = host[p.prog_off[1]:p.prog_off[1] + n_scans * J.SCAN_DTYPE.itemsize].view(J.SCAN_DTYPE)
        seen = []
        for r in srec:
            k = int(r["image"])
            o, blob = p.blobs[nb + k][0], pblobs[k]
            lo, hi = p.data_off + int(r["data_off"]), p.data_off + int(r["data_end"])
            assert o <= lo <= hi <= o + len(blob)
            seen.append((k, lo - o, hi - o))
        assert sorted(seen) == sorted((k, s.data_offset, s.data_end) for k, h in enumerate(phdrs) for s in h.scans)


@pytest.mark.parametrize("case", CASES)
def test_output_layout(case):
    blobs, pblobs, scales = CASES[case]
    hdrs, phdrs, p = plan_of(blobs, pblobs, scales)
    nb = len(hdrs)
    nbytes = [w * h * 3 for w, h in (J.scaled_size((h.width, h.height), s) for h, s in zip(hdrs + phdrs, scales))]
    assert len(p.out_offs) == len(nbytes) and p.out_offs[0] == 0
    for a, n, b in zip(p.out_offs, nbytes, p.out_offs[1:]):
        assert a + n <= b
    assert p.out_offs[-1] + nbytes[-1] == p.out_bytes + p.pout_bytes
    assert p.out_bytes == sum(nbytes[:nb]) and p.pout_bytes == sum(nbytes[nb:])
    # the records carry the same places, the progressive ones relative to the start of their part of the output
    if nb:
        assert list(p.sections[0][1]["out_off"]) == p.out_offs[:nb]
    if phdrs:
        prec = dict(p.sections)[p.prog_off[0]]
        assert [p.out_bytes + int(o) for o in prec["out_off"]] == p.out_offs[nb:]
        assert p.coef_off == [int(o) for o in prec["coef_off"]] + [p.ptot["total_blocks"]]
    else:
        assert p.coef_off == []
