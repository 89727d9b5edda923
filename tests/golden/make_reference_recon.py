"""Writes tests/golden/reference_recon.json: what the reference decoder (oracle/_ref/mini_thumbnailer_ref, built by
__graft_entry__.build() from an upstream MiniVideo checkout) gives for the corpus of tests/refcorpus.py and for its CLI
scenarios.  Per case: the generator arguments, the md5 of the stream and, per picture, the md5 of the reference's yuv420 file
and of the pixels of its BMP (RGB, top row first).  Per CLI scenario: the md5 of the input (and of what the reference is
given: Annex B for an MP4 scenario, tests/refcorpus.py) and, per file the reference wrote, the md5 of its bytes (PNG: of its
pixels).

    python tests/golden/make_reference_recon.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import refcorpus, refdec  # noqa: E402


def main():
    if not refdec.available():
        sys.exit(refdec.HOW_TO_BUILD)
    cases = {}
    for case in refcorpus.CORPUS:
        stream, _ = refcorpus.make(case)
        pics = refcorpus.reference_pictures(case, stream)
        cases[case["id"]] = {"args": {k: v for k, v in case.items() if k != "id"}, "stream_md5": refcorpus.md5(stream),
                             "pictures": [{"yuv420": refcorpus.md5(y), "bmp_rgb": refcorpus.md5(px)} for y, px in pics]}
    cli = {}
    for scn in refcorpus.CLI_SCENARIOS:
        name, data = refcorpus.cli_input(scn, for_reference=True)
        r, files = refdec.run_cli(refdec.REF_CLI, data, name, fmt=scn["fmt"], n=scn["n"], mode=scn["mode"])
        assert (r.returncode != 0) == bool(scn.get("prefix")) and files, (scn["id"], r.returncode, sorted(files))
        cli[scn["id"]] = {"scenario": scn, "input_md5": refcorpus.md5(refcorpus.cli_input(scn)[1]),
                          "reference_input_md5": refcorpus.md5(data), "returncode": r.returncode,
                          "files": refcorpus.cli_digests(files)}
    out = {"about": "reference decoder (upstream MiniVideo mini_thumbnailer, static build) on tests/refcorpus.py; "
                    "written by tests/golden/make_reference_recon.py",
           "cases": cases, "cli": cli}
    with open(refcorpus.GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d cases, %d pictures, %d CLI scenarios, %d bytes" % (
        refcorpus.GOLDEN, len(cases), sum(len(c["pictures"]) for c in cases.values()), len(cli), os.path.getsize(refcorpus.GOLDEN)))


if __name__ == "__main__":
    main()
