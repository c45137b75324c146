"""The refusal census (tools/refusal_census.py) against its recording (tests/golden/refusal_census.json): what the command line, the
drivers' check_* functions and the two drivers say to combinations of features -- every refusal's whole text and which one comes first
-- is what it was when the recording was made.  Here: every single flag and every pair of the command line, every tenth triple, and
all of the checks' and the drivers' sections; `python tools/refusal_census.py --check` runs every triple.  No device is touched."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIPLE_STEP = 10


@pytest.fixture(scope="module")
def census():
    spec = importlib.util.spec_from_file_location("refusal_census", os.path.join(ROOT, "tools", "refusal_census.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(tool.GOLDEN) as f:
        golden = json.load(f)
    assert golden["cli_atoms"] == tool.CLI_ATOMS
    outcomes, sections = tool.census(cli_triple_step=TRIPLE_STEP)
    return golden, outcomes, sections, tool.LABELS


@pytest.mark.parametrize("section", ["cli", "checks", "render_image", "render_video"])
def test_every_case_of_a_section_says_what_it_said(census, section):
    golden, outcomes, sections, labels = census
    want, got = golden["sections"][section], sections[section]
    assert len(got) == len(want)
    ran = [i for i in range(len(got)) if got[i] is not None]
    assert len(ran) == len(got) if section != "cli" else len(ran) > len(got) // TRIPLE_STEP
    differences = [(labels[section][i], golden["outcomes"][want[i]], outcomes[got[i]]) for i in ran if golden["outcomes"][want[i]] != outcomes[got[i]]]
    assert not differences, f"{len(differences)} of {len(ran)} cases differ; the first (case, recorded, now): {differences[:5]}"


def test_the_accepted_video_lines_under_two_ranks(census):
    golden, outcomes, sections, labels = census
    # (the lines of this section are the accepted --video lines among those that were run: compared by their command line)
    recorded = {}
    cli, ranks = golden["sections"]["cli"], iter(golden["sections"]["cli_ranks"])
    for argv, i in zip(labels["cli"], cli):
        if golden["outcomes"][i].startswith("ok:") and "--video" in argv:
            recorded[" ".join(argv)] = golden["outcomes"][next(ranks)]
    assert next(ranks, None) is None
    got = {" ".join(argv): outcomes[i] for argv, i in zip(labels["cli_ranks"], sections["cli_ranks"])}
    assert got and all(recorded[line] == said for line, said in got.items()), [(line, recorded[line], said) for line, said in got.items() if recorded[line] != said][:5]
