"""The variant bit that keeps the few-blocks path's wave tiles whole has one value in the host API and in the public header
(no GPU)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_bit_18_has_one_value():
    api = _read("trieste_amd", "csrc", "tgp_api.hip")
    header = _read("include", "tgp.h")
    names = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"\b(VARIANT_\w+) = (\d+)", api))
    assert names["VARIANT_PRUNE_WHOLE_TILES"] == 1 << 18
    # written in decimal, one bit per name: the new one collides with none
    assert len(set(names.values())) == len(names) and all(v > 0 and v & (v - 1) == 0 for v in names.values())
    assert not re.search(r"\bVARIANT_\w+ = 0[xX]", api)
    doc = header[header.index("Sweep launch policy knob"): header.index("int tgp_set_variant")]
    m = re.search(r"bit 18 \((\d+)\)", doc)
    assert m and int(m.group(1)) == names["VARIANT_PRUNE_WHOLE_TILES"]
    # the comment beside the constant names the same number
    assert re.search(r"VARIANT_PRUNE_WHOLE_TILES \(%d\)" % (1 << 18), api)
