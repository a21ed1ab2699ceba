"""`phenaki_pytorch_amd.dropin.install()` rebinds the reference package's model classes before its trainers are imported (VERDICT r4
next #9, north star "drops into the existing trainers"); it must refuse once the reference package was imported."""
import sys

import pytest


def test_dropin_refuses_to_run_after_the_reference_was_imported(monkeypatch):
    import types
    from phenaki_pytorch_amd import dropin
    monkeypatch.setitem(sys.modules, 'phenaki_pytorch', types.ModuleType('phenaki_pytorch'))
    with pytest.raises(RuntimeError, match='before the first'):
        dropin.install()
