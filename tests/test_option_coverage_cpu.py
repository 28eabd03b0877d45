"""The option set is closed.  vsp_set_option refuses a name that is not in the library's table of known options (csrc/capi.hip
KNOWN_OPTIONS), so a test cannot set a name nothing reads; this file holds the table, the reads in csrc, the documentation in
include/vsp.h and the names the suite uses against one another.  It parses sources and loads no library."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vote_saver_protocol_amd", "csrc")
NAME = re.compile(r'^"([a-z0-9_]+)"$')

# options no file under tests/ names as a string literal, one line of reason each; three at most
EXEMPT = {
    "generate_precompute_window": "reached through Keypair(precompute_window=), which sets it around vsp_groth16_generate (test_gpu_prover.py, test_gpu_batch_members.py)",
}


def read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def csrc_files():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc")))


def table():
    """the names of KNOWN_OPTIONS, in order"""
    m = re.search(r"KNOWN_OPTIONS\[\]\s*=\s*\{(.*?)\};", read(os.path.join(CSRC, "capi.hip")), re.S)
    assert m, "capi.hip: no KNOWN_OPTIONS table"
    body = re.sub(r"//[^\n]*", "", m.group(1))
    names = re.findall(r'"([^"]*)"', body)
    assert names and all(re.fullmatch(r"[a-z0-9_]+", n) for n in names), names
    return names


def calls(text, fn):
    """the argument lists of every call fn(...) in text, split at the top-level commas (string literals and nested parentheses kept whole)"""
    out = []
    for m in re.finditer(r"\b%s\(" % fn, text):
        args, cur, depth, i, quote = [], "", 0, m.end(), False
        while i < len(text):
            ch = text[i]
            if quote:
                cur += ch
                if ch == "\\":
                    cur += text[i + 1]; i += 1
                elif ch == '"':
                    quote = False
            elif ch == '"':
                quote = True; cur += ch
            elif ch in "([{":
                depth += 1; cur += ch
            elif ch in ")]}":
                if depth == 0:
                    break
                depth -= 1; cur += ch
            elif ch == "," and depth == 0:
                args.append(cur.strip()); cur = ""
            else:
                cur += ch
            i += 1
        args.append(cur.strip())
        out.append(args)
    return out


def names_read():
    """option name -> files that read it: the second argument of opt(ctx, "name", default); the fault hook and the switched-off option of
    record_verdict(ctx, state, same, "fault", stat, "off", msg).  A name that is not a literal could not be held against the table: only the
    two lines of common.h that define the helpers may pass one on."""
    found, computed = {}, []
    for path in csrc_files():
        text = re.sub(r"//[^\n]*", "", read(path))
        base = os.path.basename(path)
        for fn, positions in (("opt", (1,)), ("record_verdict", (3, 5))):
            for args in calls(text, fn):
                got = [NAME.match(args[p]) if p < len(args) else None for p in positions]
                if not all(got):
                    computed.append((base, fn, tuple(args)))
                for m in filter(None, got):
                    found.setdefault(m.group(1), set()).add(base)
    return found, computed


def test_the_parser_sees_the_reads_it_is_meant_to_see():
    assert calls('x = opt(ctx, "a_b", f(1, 2)) + opt(ctx, name, 0);', "opt") == [["ctx", '"a_b"', "f(1, 2)"], ["ctx", "name", "0"]]
    found, computed = names_read()
    assert "msm_window_bits" in found and "msm_fp28_selfcheck_fault" in found and "ntt_fr29" in found and len(found) > 40
    # the helpers' own definitions, and nothing else, name an option through a variable
    assert sorted((b, fn) for b, fn, _ in computed) == [("common.h", "opt"), ("common.h", "opt"), ("common.h", "record_verdict")], computed


def test_every_option_read_is_in_the_table_and_every_entry_is_read():
    names = table()
    assert len(names) == len(set(names)), "an option is listed twice"
    found, _ = names_read()
    assert sorted(set(found) - set(names)) == [], "read in csrc but refused by vsp_set_option"
    assert sorted(set(names) - set(found)) == [], "in the table but read nowhere: setting it tests nothing"


def test_every_option_is_documented_in_the_header():
    header = read(os.path.join(ROOT, "include", "vsp.h"))
    assert [n for n in table() if '"%s"' % n not in header] == []


def test_every_option_is_named_by_a_test():
    here = os.path.abspath(__file__)
    texts = []
    for d, _, files in os.walk(os.path.join(ROOT, "tests")):
        texts += [read(os.path.join(d, f)) for f in files if f.endswith(".py") and os.path.join(d, f) != here]
    suite = "\n".join(texts)
    unnamed = [n for n in table() if not re.search(r"""["']%s["']""" % n, suite)]
    assert len(EXEMPT) <= 3 and all(reason.strip() for reason in EXEMPT.values())
    assert set(EXEMPT) <= set(table()), "an exemption for a name that is no option"
    assert sorted(unnamed) == sorted(EXEMPT), "options no test sets (or exemptions no longer needed)"
    # the variants this suite was once blind to stay off the list
    assert not set(EXEMPT) & {"msm_accum28_asm", "msm_fused_split", "msm_fused_scans", "msm_dimsum_maxw", "msm_wide_windows", "msm_debug_counts",
                              "prove_host_threads", "prove_fixed_base"}
