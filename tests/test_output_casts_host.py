"""No GPU: the three statements of the output-cast contract in output_cast_refs.py agree with each other, the pattern lists
reach every class of value, and each of four wrong casts is told apart from the right one by at least one pattern of every
format it changes — which is what makes test_output_casts_gpu.py (the same patterns, the same references, the same
comparison) fail for a kernel that is wrong in one of those ways."""
import pytest
import torch

import output_cast_refs as OC


def _describe(fmt, words, got, want, bad):
    return [(hex(words[i]), [hex(int(v)) for v in got[i].reshape(-1)], [hex(int(v)) for v in want[i].reshape(-1)])
            for i in bad.nonzero().flatten().tolist()]


@pytest.mark.parametrize("fmt", OC.FORMATS)
def test_torch_reference_equals_integer_model(fmt):
    words = OC.PATTERNS[fmt]
    x = OC.values(words)
    assert [int(v) & 0xFFFFFFFF for v in x.view(torch.int32)] == words, "the fp32 tensor does not carry the bit patterns"
    ref, model = OC.ref_codes(fmt, x), OC.model_codes(fmt, words)
    bad = OC.mismatch(fmt, ref, model)
    assert not bool(bad.any()), _describe(fmt, words, ref, model, bad)
    nan = torch.tensor([OC.is_nan_bits(w) for w in words])
    assert bool((OC.is_nan_code(fmt, ref) == nan).all()) and bool((OC.is_nan_code(fmt, model) == nan).all())


@pytest.mark.parametrize("fmt", OC.FORMATS)
def test_reference_values_at_the_edges(fmt):
    """A few results written out by hand (from the formats' definitions), so that reference and model cannot be wrong together."""
    by_hand = {
        "bf16": {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x7F7F7FFF: 0x7F7F, 0x7F7F8000: 0x7F80, 0xFF800000: 0xFF80,
                 0x007FFFFF: 0x0080},
        "fp16": {OC.f32_bits(65504.0): 0x7BFF, OC.f32_bits(65520.0) - 1: 0x7BFF, OC.f32_bits(65520.0): 0x7C00,
                 OC.f32_bits(2.0 ** -24): 0x0001, OC.f32_bits(2.0 ** -25): 0x0000, OC.f32_bits(2.0 ** -25) + 1: 0x0001,
                 OC.f32_bits(1.5 * 2.0 ** -24): 0x0002, 0x3F801000: 0x3C00, 0x3F803000: 0x3C02, 0xFF800000: 0xFC00},
        "e4m3": {OC.f32_bits(448.0): 0x7E, OC.f32_bits(464.0): 0x7E, OC.f32_bits(465.0): 0x7E, OC.f32_bits(1e9): 0x7E,
                 0x7F800000: 0x7E, 0xFF800000: 0xFE, OC.f32_bits(-465.0): 0xFE, OC.f32_bits(1.0625): 0x38, OC.f32_bits(1.1875): 0x3A,
                 OC.f32_bits(17.0): 0x58, OC.f32_bits(19.0): 0x5A, OC.f32_bits(2.0 ** -9): 0x01, OC.f32_bits(2.0 ** -10): 0x00,
                 OC.f32_bits(2.0 ** -10) + 1: 0x01, OC.f32_bits(7 * 2.0 ** -9): 0x07, OC.f32_bits(7.5 * 2.0 ** -9): 0x08,
                 OC.f32_bits(432.0): 0x7E},
    }
    if fmt == "h2":
        words = [OC.f32_bits(65504.0), OC.f32_bits(1e9), 0xFF800000, OC.f32_bits(65520.0) - 1, OC.f32_bits(1.0 + 2.0 ** -12 + 2.0 ** -20)]
        want = torch.tensor([[0x7BFF, 0], [0x7BFF, 0], [0xFBFF, 0], [0x7BFF, 0], [0x3C00, 0x0C04]])   # lo = 2^-12 · (1 + 2^-8)
    else:
        words = list(by_hand[fmt])
        want = torch.tensor([by_hand[fmt][w] for w in words])
        assert set(words) <= set(OC.PATTERNS[fmt])
    for got in (OC.ref_codes(fmt, OC.values(words)), OC.model_codes(fmt, words)):
        bad = OC.mismatch(fmt, got, want)
        assert not bool(bad.any()), _describe(fmt, words, got, want, bad)


@pytest.mark.parametrize("name", list(OC.MUTATIONS))
def test_every_mutation_is_caught_by_every_format_it_changes(name):
    kwargs, formats = OC.MUTATIONS[name]
    for fmt in OC.FORMATS:
        words = OC.PATTERNS[fmt]
        bad = OC.mismatch(fmt, OC.model_codes(fmt, words, **kwargs), OC.ref_codes(fmt, OC.values(words)))
        if fmt in formats:
            assert bool(bad.any()), f"{name}: no pattern of the {fmt} list tells it from the reference"
        else:
            assert not bool(bad.any()), f"{name} is not supposed to change {fmt}"
        # the ReLU launches leave the NaN patterns out: what they can still tell apart must not depend on a NaN
        if fmt in formats and name != "NaN -> -limit":
            assert bool(bad[[not OC.is_nan_bits(w) for w in words]].any()), (name, fmt)


@pytest.mark.parametrize("fmt", OC.FORMATS)
def test_pattern_list_reaches_every_class(fmt):
    seen = {}
    for w in OC.PATTERNS[fmt]:
        if OC.is_nan_bits(w):
            seen.setdefault("nan", []).append(w)
            continue
        for c in OC.classify(fmt, w):
            seen.setdefault(c, []).append(w)
    assert set(seen) == set(OC.CLASSES), f"{fmt}: no pattern of class {set(OC.CLASSES) - set(seen)}"
    for c in ("tie-even", "tie-odd", "limit", "past-limit", "inf"):          # both signs of each
        assert {w >> 31 for w in seen[c]} == {0, 1}, (fmt, c)
    # a tie in the subnormal range as well as in the normal one
    sub = set(seen["subnormal"])
    assert any(w in sub for w in seen["tie-even"] + seen["tie-odd"]), fmt
    assert any(w not in sub for w in seen["tie-even"]) and any(w not in sub for w in seen["tie-odd"]), fmt
    assert len(set(OC.PATTERNS[fmt])) == len(OC.PATTERNS[fmt])


def test_classes_of_known_values():
    assert OC.classify("e4m3", OC.f32_bits(464.0)) == {"past-limit"}          # saturates: not a tie of the format
    assert OC.classify("e4m3", OC.f32_bits(432.0)) == {"tie-odd", "limit"}
    assert OC.classify("e4m3", OC.f32_bits(1.0625)) == {"tie-even"}
    assert OC.classify("e4m3", OC.f32_bits(2.0 ** -10)) == {"tie-even", "subnormal"}
    assert OC.classify("fp16", OC.f32_bits(65520.0)) == {"past-limit"}
    assert OC.classify("fp16", OC.f32_bits(65520.0) - 1) == {"limit"}
    assert OC.classify("h2", OC.f32_bits(65520.0) - 1) == {"past-limit"}      # the clamp comes first: saturates to 65504
    assert OC.classify("bf16", 0x7F7F8000) == {"past-limit"}
    assert OC.classify("bf16", 0x3F818000) == {"tie-odd"}
    assert OC.classify("bf16", 0x3F800000) == set()


def test_rotated_rows():
    for fmt in OC.FORMATS:
        P = len(OC.PATTERNS[fmt])
        x = OC.rotated(fmt, P + 3, r=5)
        assert [int(v) & 0xFFFFFFFF for v in x.view(torch.int32)] == [OC.PATTERNS[fmt][(i + 5) % P] for i in range(P + 3)]
        assert not bool(torch.isnan(OC.rotated(fmt, 3 * P, r=1, nan=False)).any())
