"""Fixtures for the CLIP tokenizer (vipant_amd/tokenizer.py), from the REFERENCE's own `clip/simple_tokenizer.py`.

    python tests/golden/make_golden_tokenizer.py /path/to/reference
        # writes tests/golden/bpe_simple_vocab_16e6.head.txt.gz and tests/golden/tokenizer.json (data only)

The reference's simple_tokenizer.py is loaded by file path with a stub `ftfy` whose `fix_text` is the identity: exact for the strings
below, which are ASCII or well-formed NFC text that ftfy leaves alone.

bpe_simple_vocab_16e6.head.txt.gz: the part of the reference's vocabulary file that its tokenizer reads -- the header line and the
49152 - 256 - 2 = 48894 merges behind it (simple_tokenizer.py:66-67 slices `[1 : 48895]` off the 262146 lines) -- gzipped again with
no time stamp.  The whole file is 1.36 MB, over the size limit of a committed file; the head is 0.2 MB and gives the same tokenizer:
tokenizer.json is written by the reference's tokenizer over the WHOLE file, and the script checks that the same class over the head
gives the same ids before it writes anything.

tokenizer.json: {"sot", "eot", "cases": [{"text", "ids" (encode), "clean" (what encode tokenized), "decoded" (decode(ids))}]}.
"""
import gzip
import importlib.util
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
HEAD = os.path.join(HERE, "bpe_simple_vocab_16e6.head.txt.gz")
NLINES = 49152 - 256 - 2 + 1          # the header and the merges

TEXTS = [
    "A man speaks while a dog barks in the background",
    "a woman talks nearby as water pours",
    "Rain falls and thunder roars in the distance.",
    "An engine idling, then revving up several times",
    "birds chirping and a rooster crowing while wind blows into a microphone",
    "A child laughs; an adult male speaks, followed by applause",
    "Food is frying while a woman speaks",
    "the sound of a train horn blowing as a train passes by",
    "a duck quacks continuously",
    "Someone snores loudly and then a clock ticks",
    "it's the dog's bowl", "I can't and won't", "they're here, we've won", "I'm sure she'll say he'd go",
    "IT'S THE DOG'S, THEY'RE, WE'VE, I'M, SHE'LL, HE'D",
    "room 237 at 10:45", "1234567890", "3.14159 and 2,718", "year2021model",
    "wait... what?!", "!!!???", "a -- b ;; c", "(beep) [buzz] {hum}", "#hashtag @mention $5.00 50% a&b a*b",
    "a   lot    of     blanks", "tabs\tand\nnewlines\r\n and \t mixed  \n  runs", "   leading and trailing   ",
    "ALL UPPER CASE WORDS", "MiXeD CaSe", "Tom &amp; Jerry", "Tom &amp;amp; Jerry", "a &lt;b&gt; tag &quot;quoted&quot;",
    "café au lait", "größe und straße", "naïve fiancée", "ångström ñandú",
    "xqzjvkw", "zzzzqqqqxxxx", "",
    "a", "<|startoftext|> hello <|endoftext|>",
    " ".join(["a dog barks and a cat meows while rain falls"] * 9),          # more than 77 tokens
]


def load_reference_tokenizer(root):
    sys.modules["ftfy"] = types.ModuleType("ftfy")
    sys.modules["ftfy"].fix_text = lambda text: text
    path = os.path.join(root, "clip", "simple_tokenizer.py")
    spec = importlib.util.spec_from_file_location("reference_simple_tokenizer", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["reference_simple_tokenizer"] = mod
    spec.loader.exec_module(mod)
    return mod


def write_head(root):
    with gzip.open(os.path.join(root, "clip", "bpe_simple_vocab_16e6.txt.gz")) as f:
        lines = f.read().decode("utf-8").split("\n")
    with open(HEAD, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, compresslevel=9, mtime=0) as f:
        f.write(("\n".join(lines[:NLINES]) + "\n").encode("utf-8"))
    return len(lines)


def main(root):
    ref = load_reference_tokenizer(root)
    whole = ref.SimpleTokenizer(os.path.join(root, "clip", "bpe_simple_vocab_16e6.txt.gz"))
    nlines = write_head(root)
    head = ref.SimpleTokenizer(HEAD)
    assert head.encoder == whole.encoder and head.bpe_ranks == whole.bpe_ranks
    cases = []
    for text in TEXTS:
        ids = whole.encode(text)
        assert head.encode(text) == ids
        cases.append({"text": text, "ids": ids, "clean": ref.whitespace_clean(ref.basic_clean(text)).lower(), "decoded": whole.decode(ids)})
    out = {"sot": whole.encoder["<|startoftext|>"], "eot": whole.encoder["<|endoftext|>"], "cases": cases}
    with open(os.path.join(HERE, "tokenizer.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"vocabulary: {nlines} lines, {NLINES} kept ({os.path.getsize(HEAD)} bytes); {len(cases)} strings, "
          f"longest {max(len(c['ids']) for c in cases)} ids")


if __name__ == "__main__":
    main(sys.argv[1])
