"""The CLIP byte-pair tokenizer on the host (vipant_amd/tokenizer.py) against what the reference's own `SimpleTokenizer` recorded
(tests/golden/tokenizer.json, made by tests/golden/make_golden_tokenizer.py with `ftfy` = identity over the WHOLE vocabulary file), read
here from the head of that file (tests/golden/bpe_simple_vocab_16e6.head.txt.gz: the merges the tokenizer reads), and `tokenize` with
the contract of clip/clip.py:171-206."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BPE = os.path.join(ROOT, "tests", "golden", "bpe_simple_vocab_16e6.head.txt.gz")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "tokenizer.json")))
CASES = GOLD["cases"]


@pytest.fixture(scope="module")
def tok():
    from vipant_amd.tokenizer import load_tokenizer
    return load_tokenizer(BPE)


def test_the_fixture_covers_what_it_says():
    texts = [c["text"] for c in CASES]
    assert len(texts) >= 40 and "" in texts and any(len(c["ids"]) > 75 for c in CASES)
    assert any("&amp;amp;" in t for t in texts) and any("\t" in t and "\n" in t for t in texts)
    assert any(not t.isascii() for t in texts) and any(t.isupper() for t in texts)
    for suffix in ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d"):
        assert any(suffix + " " in t or t.endswith(suffix) for t in texts), suffix


@pytest.mark.parametrize("case", range(len(CASES)))
def test_ids_are_the_reference_s(tok, case):
    c = CASES[case]
    assert tok.encode(c["text"]) == c["ids"], c["text"]
    assert tok.clean(c["text"]) == c["clean"]
    assert tok.decode(c["ids"]) == c["decoded"]


def test_sot_and_eot_are_the_trainer_s_constants(tok):
    import ast
    # (the constants of vipant_amd/monitor.py, read from its source: importing it would load the HIP binding)
    tree = ast.parse(open(os.path.join(ROOT, "vipant_amd", "monitor.py")).read())
    consts = [n for n in tree.body if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Tuple)
              and [e.id for e in n.targets[0].elts] == ["SOT", "EOT"]]
    assert len(consts) == 1 and ast.literal_eval(consts[0].value) == (49406, 49407)
    assert (tok.sot_token, tok.eot_token) == (49406, 49407) == (GOLD["sot"], GOLD["eot"])
    assert len(tok.encoder) == 49408 and tok.decode([49406, 49407]) == "<|startoftext|><|endoftext|>"


def test_decode_round_trips_the_cleaned_string(tok):
    # words and punctuation runs come back separated by one blank: compare blank-free, and exactly where the text has no punctuation
    for c in CASES:
        back = tok.decode(tok.encode(c["text"]))
        assert back.replace(" ", "") == c["clean"].replace(" ", ""), c["text"]
    for text in ("a woman talks nearby as water pours", "ALL UPPER CASE WORDS", "a   lot    of     blanks", "café au lait"):
        assert tok.decode(tok.encode(text)) == tok.clean(text) + " "


def test_tokenize_list_tensor_too_long_and_truncate(tok):
    from vipant_amd.tokenizer import tokenize
    texts = [c["text"] for c in CASES[:12]]
    rows = tokenize(texts, as_list=True)
    assert rows == [[49406] + c["ids"] + [49407] for c in CASES[:12]]
    assert tokenize("a dog barking", as_list=True) == tokenize(["a dog barking"], as_list=True)
    t = tokenize(texts)
    assert t.dtype == torch.int64 and t.shape == (12, 77)
    for row, want in zip(t.tolist(), rows):
        assert row[:len(want)] == want and not any(row[len(want):])
    assert tokenize(texts, context_length=32).shape == (12, 32)
    assert tokenize("").tolist() == [[49406, 49407] + [0] * 75]
    long = next(c for c in CASES if len(c["ids"]) > 75)
    with pytest.raises(RuntimeError, match="is too long for context length 77"):
        tokenize([texts[0], long["text"]])
    cut = tokenize([texts[0], long["text"]], truncate=True)
    assert cut.shape == (2, 77) and cut[1].tolist() == [49406] + long["ids"][:75] + [49407]
    assert cut[0].tolist()[:len(rows[0])] == rows[0]
    # a tokenizer passed in is the one used
    assert tokenize("rain", as_list=True, tokenizer=tok) == [[49406] + tok.encode("rain") + [49407]]


def test_without_ftfy_one_warning_for_text_outside_ascii(tok, monkeypatch):
    import warnings
    from vipant_amd import tokenizer as TK
    monkeypatch.setattr(TK, "ftfy", None)
    monkeypatch.setattr(TK, "_warned_ftfy", False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tok.encode("plain ascii text")                                      # nothing to warn about
    with pytest.warns(UserWarning, match="ftfy is not installed"):
        ids = tok.encode("café au lait")
    assert ids == next(c["ids"] for c in CASES if c["text"] == "café au lait")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tok.encode("größe und straße")                                      # once
    calls = []
    monkeypatch.setattr(TK, "ftfy", type("F", (), {"fix_text": staticmethod(lambda t: calls.append(t) or t)}))
    assert tok.encode("naïve fiancée") == next(c["ids"] for c in CASES if c["text"] == "naïve fiancée") and calls == ["naïve fiancée"]


def test_where_the_vocabulary_file_comes_from(tmp_path):
    import shutil
    from vipant_amd.config import to_config
    from vipant_amd.errors import VipantError
    from vipant_amd.tokenizer import BPE_FILE, SimpleTokenizer, load_tokenizer, resolve_bpe_path
    assert BPE_FILE == "bpe_simple_vocab_16e6.txt.gz"
    clip_root, data_root = tmp_path / "clip", tmp_path / "data"
    clip_root.mkdir(), data_root.mkdir()
    rcfg = to_config(dict(bpe_path="", clip_model_root=str(clip_root), data_root=str(data_root)))
    with pytest.raises(VipantError, match=r"running\.bpe_path"):
        resolve_bpe_path(rcfg)
    with pytest.raises(VipantError, match=r"running\.bpe_path"):
        load_tokenizer(rcfg)
    with pytest.raises(VipantError, match=r"running\.bpe_path"):
        SimpleTokenizer(str(tmp_path / "none.txt.gz"))
    shutil.copy(BPE, data_root / BPE_FILE)
    assert resolve_bpe_path(rcfg) == f"{data_root}/{BPE_FILE}"
    shutil.copy(BPE, clip_root / BPE_FILE)
    assert resolve_bpe_path(rcfg) == f"{clip_root}/{BPE_FILE}"              # clip_model_root before data_root
    rcfg.bpe_path = BPE
    assert resolve_bpe_path(rcfg) == BPE                                    # the key before both
    assert load_tokenizer(rcfg) is load_tokenizer(BPE)                      # one tokenizer per file
    rcfg.bpe_path = str(tmp_path / "none.txt.gz")                           # a path that does not exist falls through
    assert resolve_bpe_path(rcfg) == f"{clip_root}/{BPE_FILE}"
    from vipant_amd.config_defaults import GROUPS
    assert all(group["bpe_path"] == "" for group in GROUPS["running"].values())        # the key's default, in every running group
    # a file that is not the vocabulary
    import gzip
    with gzip.open(tmp_path / "short.txt.gz", "wb") as f:
        f.write(b"#version\na b\n")
    with pytest.raises(VipantError, match="does not hold the 48894 merges"):
        SimpleTokenizer(str(tmp_path / "short.txt.gz"))


def test_importing_the_package_opens_no_vocabulary_file():
    code = ("import builtins, gzip, sys\n"
            "opened = []\n"
            "real_open, real_gzip = builtins.open, gzip.open\n"
            "def spy(path, *a, **k):\n"
            "    opened.append(str(path)); return real_open(path, *a, **k)\n"
            "def gzspy(path, *a, **k):\n"
            "    opened.append(str(path)); return real_gzip(path, *a, **k)\n"
            "builtins.open, gzip.open = spy, gzspy\n"
            "import vipant_amd, cvap, vipant_amd.data\n"
            "from vipant_amd import SimpleTokenizer, tokenize\n"
            "assert cvap.tokenize is vipant_amd.tokenize is vipant_amd.tokenizer.tokenize\n"
            "assert cvap.SimpleTokenizer is SimpleTokenizer\n"
            "assert not [p for p in opened if 'bpe' in p or p.endswith('.gz')], opened\n"
            "assert vipant_amd.tokenizer._tokenizer is None\n"
            "assert 'vipant_amd._ffi' not in sys.modules and 'clip' not in sys.modules\n"
            "try:\n"
            "    tokenize('a dog')\n"
            "except vipant_amd.errors.VipantError as e:\n"
            "    assert 'running.bpe_path' in str(e)\n"
            "else:\n"
            "    raise AssertionError('tokenize without a vocabulary did not raise')\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
