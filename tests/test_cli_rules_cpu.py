"""Which refusal wins: every subset of up to three of nineteen flag tokens, recorded from main() before its if-chain became the ordered table
main.FLAG_RULES (tests/golden/cli_refusals.json: {'messages': [...], 'cases': [[argv, index into messages], ...]}), replayed against main().
Every case names device 99, which no machine has, so each one ends in a SystemExit before an engine is built: a case that passes every
rule ends in the device message, whose count of visible devices is this machine's."""
import argparse
import json
import os

import torch

import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import main as M

HERE = os.path.dirname(os.path.abspath(__file__))


def test_every_recorded_refusal_is_reproduced():
    with open(os.path.join(HERE, 'golden', 'cli_refusals.json')) as fh:
        doc = json.load(fh)
    recorded = '--gpus [99]: device 99 does not exist (0 visible)'      # the recording machine had no device
    assert recorded in doc['messages'] and len(doc['cases']) == 1108
    here = recorded.replace('(0 visible)', '(%d visible)' % torch.cuda.device_count())
    keep = argparse.Namespace(**vars(M.hps))
    wrong = []
    for argv, m in doc['cases']:
        want = doc['messages'][m]
        try:
            M.main(list(argv))
            got = None
        except SystemExit as e:
            got = e.code
        finally:
            M.hps = keep
        if got != (here if want == recorded else want):
            wrong.append((argv, want, got))
    assert not wrong, '%d of %d cases differ; the first: %r' % (len(wrong), len(doc['cases']), wrong[0])
