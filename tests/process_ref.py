"""The model of default_process: rapidfuzz's pure-Python processor made context-free.

m(c) is U+0020 when re.match(r"\\W", c) matches (c is neither str.isalnum nor "_"), else c.lower()[0]; default_process maps every
scalar value with m and removes U+0020 from both ends (inner runs of spaces stay).  It differs from the whole-string form
re.sub(r"(?ui)\\W", " ", s).strip().lower() in two places only: U+03A3 in final-sigma position (whole string: U+03C2, here: U+03C3)
and U+0130 (whole string: "i" + U+0307, here: "i").
"""
import re

_NON_WORD = re.compile(r"\W")
_NON_WORD_WHOLE = re.compile(r"(?ui)\W")


def map_char(c):
    """m(c) for a string of one scalar value."""
    if _NON_WORD.match(c):
        return " "
    return c.lower()[0]


def map_cp(cp):
    """m as a function of code points; surrogates and values above U+10FFFF map to U+0020."""
    if cp > 0x10FFFF or 0xD800 <= cp <= 0xDFFF:
        return 0x20
    return ord(map_char(chr(cp)))


def default_process(s):
    if s is None:
        return None
    return "".join(map_char(c) for c in s).strip(" ")


def default_process_whole(s):
    """rapidfuzz's pure-Python default_process (the whole-string form)."""
    return _NON_WORD_WHOLE.sub(" ", s).strip().lower()


def default_process_column(col):
    return [default_process(s) for s in col]
