"""The cooperative reset (csrc/skyjo_record.h) works on lanes that the surrounding code has switched off: its registers must be the
same from the reserve at the top of an iteration to the release at its end, and nothing else may write them in between.  That is a
property of the compiler's output, so it is checked there, for every kernel that holds the pair (tools/check_coop_regs.py)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_reserved_registers_in_every_instantiation():
    import check_coop_regs as c

    found, bad = c.check(c.compile_unit())
    assert found == 12, found  # k_cycle and k_step<.., true, ..> at three and four players, both observations, both layouts
    assert not bad, "\n".join(bad)
