"""The variant bit that keeps the scalar pre-screen has one value in the host API and in the public header (no GPU)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_bit_16_has_one_value():
    api = _read("trieste_amd", "csrc", "tgp_api.hip")
    header = _read("include", "tgp.h")
    names = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"\b(VARIANT_\w+) = (\d+)", api))
    assert names["VARIANT_PRESCREEN_SCALAR"] == 1 << 16
    assert names["VARIANT_PRUNE_NO_FEW"] == 1 << 15
    # one bit per name: the new one collides with none
    assert len(set(names.values())) == len(names) and all(v & (v - 1) == 0 for v in names.values())
    doc = header[header.index("Sweep launch policy knob"): header.index("int tgp_set_variant")]
    m = re.search(r"bit 16 \((\d+)\)", doc)
    assert m and int(m.group(1)) == names["VARIANT_PRESCREEN_SCALAR"]
    # the comment beside the constant names the same number
    assert re.search(r"VARIANT_PRESCREEN_SCALAR \(%d\)" % (1 << 16), api)
