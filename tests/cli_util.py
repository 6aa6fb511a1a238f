"""The command line in a fresh process, for the tests that run it end to end."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_cli(args, cwd, timeout=600):
    """`python -m joint_cnn_mrf_amd.main ARGS` in directory cwd, the package taken from this tree -> the CompletedProcess (text captured).  The
    caller asserts on returncode."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, '-m', 'joint_cnn_mrf_amd.main'] + list(args), cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
