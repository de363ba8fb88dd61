"""CPU tier: the blob layouts are an on-disk contract -- a saved blob depends on the order and the offsets of its
tensors, not only on their names and shapes.  tests/golden/blob_layout_digests.json holds a SHA-256 per layout, recorded
from the library before the layouts were rebuilt on Layout::add_conv: every MODEL_CONFIGS entry at n_vocab = 100 with 1
and 4 speakers, and its posterior encoder's layout at 513 and 80 spectrogram channels."""
import hashlib
import json
import os

import pytest

from wetts_amd import checkpoint, config

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blob_layout_digests.json")) as _f:
    DIGESTS = json.load(_f)


def _digest(layout, numel):
    """SHA-256 over the blob's size and every tensor's name, offset, numel and shape, in layout order."""
    doc = {"numel": numel, "tensors": [[n, off, num, list(shape)] for n, off, num, shape in layout]}
    return hashlib.sha256(json.dumps(doc, separators=(",", ":")).encode()).hexdigest()


def _cfg(key):
    mname, spk = key.split("/")[:2]
    return config.make_config(config.MODEL_CONFIGS[mname], 100, int(spk[len("spk"):]))


def test_digest_file_covers_every_config():
    want = {f"{m}/spk{n}" for m in config.MODEL_CONFIGS for n in (1, 4)}
    assert set(DIGESTS["main"]) == want
    assert set(DIGESTS["posterior"]) == {f"{k}/spec{s}" for k in want for s in (513, 80)}


@pytest.mark.parametrize("key", sorted(DIGESTS["main"]))
def test_blob_layout_digest(key):
    cfg = _cfg(key)
    assert _digest(checkpoint.blob_layout(cfg), checkpoint.blob_numel(cfg)) == DIGESTS["main"][key]


@pytest.mark.parametrize("key", sorted(DIGESTS["posterior"]))
def test_posterior_layout_digest(key):
    cfg, spec = _cfg(key), int(key.split("/")[2][len("spec"):])
    assert _digest(checkpoint.posterior_layout(cfg, spec), checkpoint.posterior_numel(cfg, spec)) == \
        DIGESTS["posterior"][key]
