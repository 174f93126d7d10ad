"""vipant_amd -- MI355X (gfx950) native hot path of VIP-ANT's bimodal contrastive training step.

Host side mirrors the reference's operator API (`cvap.module`, `cvap.model`, `train.py`); all numerics run in
hand-written HIP kernels behind the C ABI in include/vipant_hip.h (vipant_amd/lib/libvipant_hip.so).
"""
__version__ = "0.1.0"


def __getattr__(name):
    """`vipant_amd.tokenize`, `SimpleTokenizer`, `load_tokenizer` (vipant_amd/tokenizer.py; host only): resolved on first use, so that
    importing the package needs neither the `regex` module nor a vocabulary file."""
    if name in ("SimpleTokenizer", "load_tokenizer", "tokenize"):
        from . import tokenizer
        return getattr(tokenizer, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
