"""tools/patches/train_ff_knobs_and_ablations.patch puts the frozen tuning knobs and timing ablations of the training feed-forward kernels back
(tools/experiments/ab_train_variants.sh, ab_bits.sh).  It is only worth keeping while it applies to the current sources: `git apply --check` on a
copy of csrc/ and include/, outside any repository."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = os.path.join(ROOT, "tools", "patches", "train_ff_knobs_and_ablations.patch")


@pytest.mark.skipif(shutil.which("git") is None, reason="git is not on the path")
def test_the_feed_forward_knob_patch_applies_to_the_current_sources(tmp_path):
    shutil.copytree(os.path.join(ROOT, "difffacto_amd", "csrc"), tmp_path / "difffacto_amd" / "csrc")
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    env = dict(os.environ, GIT_CEILING_DIRECTORIES=str(tmp_path.parent))   # (a temporary directory inside a checkout is still "outside")
    r = subprocess.run(["git", "apply", "--check", "--verbose", PATCH], cwd=tmp_path, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
