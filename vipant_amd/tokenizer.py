"""The CLIP byte-pair tokenizer (clip/simple_tokenizer.py, `tokenize` of clip/clip.py:171-206): caption -> token ids, on the host.
Nothing here imports the HIP binding; loader workers and dataset constructors call it.

The vocabulary file (`bpe_simple_vocab_16e6.txt.gz`, the merges list of the CLIP release) is data and is not part of the package: its
path comes from the configuration (`resolve_bpe_path`), and the module-level tokenizer that `tokenize` uses is made on first use --
importing the package reads no file.

Deviation from the reference: `ftfy.fix_text` runs when `ftfy` imports; without it that step is skipped, and the first text holding a
non-ASCII character raises one warning (ASCII text, and text that is already well-formed NFC, come out the same either way).
"""
from __future__ import annotations

import gzip
import html
import os
import warnings
from functools import lru_cache

import regex as re

from .errors import VipantError

try:
    import ftfy
except ImportError:
    ftfy = None

BPE_FILE = "bpe_simple_vocab_16e6.txt.gz"
SOT_TEXT, EOT_TEXT = "<|startoftext|>", "<|endoftext|>"
_warned_ftfy = False


@lru_cache()
def bytes_to_unicode():
    """byte -> a printable unicode character: the reversible table the merges are written in (simple_tokenizer.py:16-35)."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(2 ** 8):
        if b not in bs:
            bs.append(b)
            cs.append(2 ** 8 + n)
            n += 1
    return dict(zip(bs, [chr(c) for c in cs]))


def get_pairs(word):
    """The set of adjacent symbol pairs of a word (a tuple of variable-length strings)."""
    pairs = set()
    prev_char = word[0]
    for char in word[1:]:
        pairs.add((prev_char, char))
        prev_char = char
    return pairs


def basic_clean(text):
    global _warned_ftfy
    if ftfy is not None:
        text = ftfy.fix_text(text)
    elif not _warned_ftfy and not text.isascii():
        _warned_ftfy = True
        warnings.warn("ftfy is not installed: text is tokenized without ftfy.fix_text (a non-ASCII character was seen)")
    text = html.unescape(html.unescape(text))
    return text.strip()


def whitespace_clean(text):
    text = re.sub(r"\s+", " ", text)
    return text.strip()


class SimpleTokenizer(object):
    def __init__(self, bpe_path):
        if not bpe_path or not os.path.isfile(str(bpe_path)):
            raise VipantError(f"running.bpe_path: `{bpe_path}` is not a file (the CLIP vocabulary {BPE_FILE})")
        self.byte_encoder = bytes_to_unicode()
        self.byte_decoder = {v: k for k, v in self.byte_encoder.items()}
        with gzip.open(str(bpe_path)) as f:
            merges = f.read().decode("utf-8").split("\n")
        merges = merges[1:49152 - 256 - 2 + 1]
        merges = [tuple(merge.split()) for merge in merges]
        if len(merges) != 49152 - 256 - 2 or any(len(m) != 2 for m in merges):
            raise VipantError(f"running.bpe_path: {bpe_path} does not hold the {49152 - 256 - 2} merges of the CLIP vocabulary")
        vocab = list(bytes_to_unicode().values())
        vocab = vocab + [v + "</w>" for v in vocab]
        for merge in merges:
            vocab.append("".join(merge))
        vocab.extend([SOT_TEXT, EOT_TEXT])
        self.encoder = dict(zip(vocab, range(len(vocab))))
        self.decoder = {v: k for k, v in self.encoder.items()}
        self.bpe_ranks = dict(zip(merges, range(len(merges))))
        self.cache = {SOT_TEXT: SOT_TEXT, EOT_TEXT: EOT_TEXT}
        self.pat = re.compile(r"""<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+""",
                              re.IGNORECASE)
        self.sot_token, self.eot_token = self.encoder[SOT_TEXT], self.encoder[EOT_TEXT]

    def bpe(self, token):
        if token in self.cache:
            return self.cache[token]
        word = tuple(token[:-1]) + (token[-1] + "</w>",)
        pairs = get_pairs(word)
        if not pairs:
            return token + "</w>"
        while True:
            bigram = min(pairs, key=lambda pair: self.bpe_ranks.get(pair, float("inf")))
            if bigram not in self.bpe_ranks:
                break
            first, second = bigram
            new_word = []
            i = 0
            while i < len(word):
                try:
                    j = word.index(first, i)
                    new_word.extend(word[i:j])
                    i = j
                except ValueError:
                    new_word.extend(word[i:])
                    break
                if word[i] == first and i < len(word) - 1 and word[i + 1] == second:
                    new_word.append(first + second)
                    i += 2
                else:
                    new_word.append(word[i])
                    i += 1
            word = tuple(new_word)
            if len(word) == 1:
                break
            pairs = get_pairs(word)
        word = " ".join(word)
        self.cache[token] = word
        return word

    @staticmethod
    def clean(text):
        """What `encode` tokenizes: ftfy (when installed), html.unescape twice, whitespace runs to one blank, lower case."""
        return whitespace_clean(basic_clean(text)).lower()

    def encode(self, text):
        bpe_tokens = []
        for token in re.findall(self.pat, self.clean(text)):
            token = "".join(self.byte_encoder[b] for b in token.encode("utf-8"))
            bpe_tokens.extend(self.encoder[bpe_token] for bpe_token in self.bpe(token).split(" "))
        return bpe_tokens

    def decode(self, tokens):
        text = "".join([self.decoder[token] for token in tokens])
        return bytearray([self.byte_decoder[c] for c in text]).decode("utf-8", errors="replace").replace("</w>", " ")


def resolve_bpe_path(rcfg):
    """The vocabulary file of a run: `running.bpe_path`, else the file inside `running.clip_model_root`, else inside
    `running.data_root` -- the first that exists."""
    get = rcfg.get if hasattr(rcfg, "get") else (lambda k, d=None: getattr(rcfg, k, d))
    tried = []
    for path in (get("bpe_path", ""), *(f"{get(k, '')}/{BPE_FILE}" for k in ("clip_model_root", "data_root") if get(k, ""))):
        if path:
            tried.append(str(path))
            if os.path.isfile(str(path)):
                return str(path)
    raise VipantError(f"running.bpe_path: no CLIP vocabulary file ({BPE_FILE}); tried {tried or 'nothing: no path is configured'}")


_tokenizers = {}
_tokenizer = None


def load_tokenizer(bpe_path):
    """The tokenizer over `bpe_path` (a `running` node: the path `resolve_bpe_path` finds), one per file; it becomes the module's
    tokenizer, the one `tokenize` uses when none is passed."""
    global _tokenizer
    if not isinstance(bpe_path, (str, os.PathLike)):
        bpe_path = resolve_bpe_path(bpe_path)
    key = os.path.abspath(str(bpe_path))
    if key not in _tokenizers:
        _tokenizers[key] = SimpleTokenizer(key)
    _tokenizer = _tokenizers[key]
    return _tokenizer


def tokenize(texts, context_length=77, as_list=False, truncate=False, tokenizer=None):
    """clip/clip.py:171-206.  One string or a list of strings -> `as_list`: [[SOT] + ids + [EOT], ...]; otherwise an int64 tensor
    [n, context_length], zero padded -- a text of more than `context_length` tokens raises RuntimeError unless `truncate`, which
    cuts it and ends it with EOT."""
    tokenizer = tokenizer if tokenizer is not None else _tokenizer
    if tokenizer is None:
        raise VipantError("running.bpe_path: no tokenizer is loaded (vipant_amd.tokenizer.load_tokenizer(path or the `running` node))")
    if isinstance(texts, str):
        texts = [texts]
    sot_token, eot_token = tokenizer.sot_token, tokenizer.eot_token
    all_tokens = [[sot_token] + tokenizer.encode(text) + [eot_token] for text in texts]
    if as_list:
        return all_tokens
    import torch
    result = torch.zeros(len(all_tokens), context_length, dtype=torch.long)
    for i, tokens in enumerate(all_tokens):
        if len(tokens) > context_length:
            if truncate:
                tokens = tokens[:context_length]
                tokens[-1] = eot_token
            else:
                raise RuntimeError(f"Input {texts[i]} is too long for context length {context_length}")
        result[i, :len(tokens)] = torch.tensor(tokens)
    return result
