"""The JPEG decoder's host code against tests/golden/jpeg_parse_pins.json: the answers of the two parsers to every single-byte
change and truncation of four headers, the words and refusals of the two clip planners, and the checksums of the decode tables and
scan plans, all as the commit before the host code was folded gave them (tests/golden/make_jpeg_parse_pins.py recorded them and
is what recomputes them here).  No GPU, no sanitizer."""
import importlib.util
import json
import os

import pytest

from tests import jpeg_decode_cases as DC

_spec = importlib.util.spec_from_file_location("make_jpeg_parse_pins", os.path.join(DC.GOLDEN, "make_jpeg_parse_pins.py"))
PINS = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(PINS)


@pytest.fixture(scope="module")
def fixture():
    with open(PINS.OUT) as f:
        return json.load(f)


def differing(got, want):
    return sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))


def test_the_parsers_answer_every_damaged_header_as_before(fixture):
    digests, texts = PINS.parser_pins()
    assert len(fixture["parser_digests"]) > 200
    assert differing(digests, fixture["parser_digests"]) == []      # (a key: stream / function / kind / first offset of the bucket)
    assert texts == fixture["refusal_texts"]
    assert len(texts) == fixture["refusal_text_count"] >= PINS.MIN_TEXTS


def test_the_clip_planners_give_the_same_words_and_refusals(fixture):
    words, refusals = PINS.clip_pins()
    assert len(fixture["clip_plan_words"]) == 2 * 27 and len(fixture["clip_plan_refusals"]) > 50
    assert differing(words, fixture["clip_plan_words"]) == []
    assert {k: (refusals.get(k), fixture["clip_plan_refusals"].get(k)) for k in differing(refusals, fixture["clip_plan_refusals"])} == {}


def test_the_decode_tables_and_scan_plans_have_the_same_bytes(fixture):
    sums = PINS.tool_checksums()
    assert len(fixture["table_checksums"]) > 200
    assert differing(sums, fixture["table_checksums"]) == []
