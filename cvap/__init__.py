"""Import-path compatibility: `cvap.module`, `cvap.model`, `cvap.monitor`, `cvap.util` resolve to the MI355X-native
implementations in `vipant_amd`, so code written against the reference's operator API runs unchanged.  The reference's
`from clip import tokenize` is `from cvap import tokenize` here (no top-level `clip` package: it would shadow an installed one)."""


def __getattr__(name):
    import vipant_amd
    if name in ("SimpleTokenizer", "load_tokenizer", "tokenize"):
        return getattr(vipant_amd, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
