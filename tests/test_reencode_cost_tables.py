"""alfalfa_amd/csrc/cost_tables.h equals what tools/gen_cost_tables.py reads from the reference's objects (oracle/_ref/obj: the bytes of
the bool-cost table as the reference compiles it).  Skipped where the oracle build is not there.  CPU only."""
import os
import struct

import pytest

import gen_cost_tables as g


@pytest.mark.skipif(not os.path.exists(os.path.join(g.OBJ, "enc_costs.o")), reason="oracle/_ref is not built")
def test_the_committed_header_is_what_the_reference_compiles():
    assert open(g.TARGET).read() == g.render(g.tables())


def test_the_table_has_no_closed_form_and_the_header_holds_it_whole():
    import math
    import re
    text = open(g.TARGET).read()
    start = text.index("\n", text.index("k_prob_cost[256]"))
    vals = [int(v) for v in re.findall(r"\d+", text[start:text.index("};")])]
    assert len(vals) == 256 and vals[0] == vals[1] and vals[128] == 255 and vals[255] == 1 and all(a >= b for a, b in zip(vals, vals[1:]))
    # (why it is read and not computed: the obvious expression misses some entries)
    closed = [max(1, int(math.floor(-256 * math.log2(p / 256.0))) - 1) for p in range(1, 256)]
    assert sum(a != b for a, b in zip(closed, vals[1:])) > 0


def test_the_elf_reader_refuses_what_is_not_an_object(tmp_path):
    p = tmp_path / "x.o"
    p.write_bytes(struct.pack("<16s", b"not an elf file"))
    with pytest.raises(AssertionError):
        g.symbol_bytes(str(p), "_ZL13vp8_prob_cost")
