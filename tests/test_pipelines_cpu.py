"""tests/pipelines.py without a GPU: its knob list against the library's sources, and the clean slate knobs() gives."""
import glob
import os
import re

import pytest

from tests import pipelines as P

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pais_mvs_amd", "csrc")


def test_knobs_are_the_names_the_library_reads():
    """KNOBS, as a set, is every "PAIS_..." string literal of csrc/*.hip and *.hpp (the closing quote right after the name: a
    name inside an error message is no knob); no duplicates.  A knob added to or deleted from the library must follow here."""
    read = set()
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")):
        with open(path) as f:
            read |= set(re.findall(r'"(PAIS_[A-Z0-9_]+)"', f.read()))
    assert len(read) >= 50, sorted(read)
    assert len(P.KNOBS) == len(set(P.KNOBS)), sorted(k for k in set(P.KNOBS) if P.KNOBS.count(k) > 1)
    assert set(P.KNOBS) == read, (sorted(read - set(P.KNOBS)), sorted(set(P.KNOBS) - read))
    for name, env in vars(P).items():           # every named pipeline is made of knobs
        if name.isupper() and isinstance(env, dict):
            assert set(env) <= read, (name, sorted(set(env) - read))


def _pais_env():
    return {k: v for k, v in os.environ.items() if k.startswith("PAIS_") and k in P.KNOBS}


def test_knobs_gives_a_clean_slate(monkeypatch):
    """Inside the block the library's part of the environment is exactly env, whatever was set before; after it none of env's
    names is set; a name the library does not read is refused before anything changes; the block does not nest."""
    monkeypatch.setenv("PAIS_TILE", "0")
    monkeypatch.setenv("PAIS_STREAM_ROUNDS", "2")
    monkeypatch.setenv("PAIS_PSO_RING", "0")
    env = dict(P.RING, **P.NO_PRE)
    assert "PAIS_PSO_RING" in env
    with P.knobs(monkeypatch, env):
        assert _pais_env() == env
        with pytest.raises(AssertionError, match="does not nest"):
            with P.knobs(monkeypatch, P.LITERAL):
                pass
        assert _pais_env() == env               # (the refused inner block touched nothing)
    assert not set(env) & set(os.environ) and _pais_env() == {}
    with pytest.raises(AssertionError, match="PAIS_SPLIT_ABOV"):
        with P.knobs(monkeypatch, {"PAIS_SPLIT_ABOV": "1"}):
            pass
    with pytest.raises(AssertionError, match="PAIS_NO_BUILD"):      # (read by the Python package, not by the library)
        with P.knobs(monkeypatch, {"PAIS_NO_BUILD": "1"}):
            pass
    with P.knobs(monkeypatch, {}):              # usable again after the refusals
        assert _pais_env() == {}
