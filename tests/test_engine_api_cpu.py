"""The surface of Engine, pinned: tests/golden/engine_api.json holds, for every function attribute of the class as it stood before engine.py
became the package engine/, its name, str(inspect.signature(.)) and the SHA-256 of its docstring ('' where there is none), and the names the
engine module exports.  Importing the class needs no device."""
import hashlib
import inspect
import json
import os

import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import engine

# the shared helpers the package added to the class; a later addition has to be listed here
NEW_HELPERS = {'_call', '_given_or_new', '_seq_lattice'}


def _recorded(repo_root):
    with open(os.path.join(repo_root, 'tests', 'golden', 'engine_api.json')) as fh:
        return json.load(fh)


def _functions():
    return dict(inspect.getmembers(engine.Engine, inspect.isfunction))


def test_every_recorded_function_keeps_its_signature_and_docstring(repo_root):
    rec, now = _recorded(repo_root)['functions'], _functions()
    assert len(rec) == 85
    for name, want in rec.items():
        assert name in now, name
        f = now[name]
        assert str(inspect.signature(f)) == want['signature'], name
        assert (hashlib.sha256(f.__doc__.encode()).hexdigest() if f.__doc__ else '') == want['doc_sha256'], name


def test_the_only_new_functions_are_the_shared_helpers(repo_root):
    assert set(_functions()) - set(_recorded(repo_root)['functions']) == NEW_HELPERS


def test_module_exports(repo_root):
    names = _recorded(repo_root)['module_exports']
    assert names == ['Engine', 'SEQ_EXCLUDE', '_hm_size']
    for name in names:
        assert hasattr(engine, name), name
    assert engine.SEQ_EXCLUDE is joint_cnn_mrf_amd.motion.SEQ_EXCLUDE and engine._hm_size(480) == 60
