"""
Replay the reference's OWN golden test outputs byte-for-byte.

The reference ships bash test harnesses whose `.out` files interleave
`# dn scan <args>` marker lines with the exact expected stdout
(tools/catest compares verbatim).  These tests parse those goldens,
run OUR `dn` with the same arguments against the reference's own
fixture data, and require identical output — the strongest possible
CLI-parity evidence, using goldens we did not produce.

The fixture logs and the recorded `.out` files are stored under
tests/golden/reference/, each gzipped, in the reference's own layout
(tests/data, tests/dn/local, tests/dn/manta), and unpacked into a
temporary tree for the module, so the replay needs nothing outside the
repository.
"""

import gzip
import os
import re
import subprocess

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                      "golden", "reference")
REF = None   # <unpacked tree>/tests, set by reference_tree
DATA = None  # REF/data


@pytest.fixture(scope="module", autouse=True)
def reference_tree(tmp_path_factory):
    """Unpack tests/golden/reference/**.gz, byte for byte, into a
    temporary tree of the same layout."""
    global REF, DATA
    root = str(tmp_path_factory.mktemp("reference"))
    nfiles = 0
    for dirpath, _dirs, names in os.walk(GOLDEN):
        dest = os.path.join(root, os.path.relpath(dirpath, GOLDEN))
        os.makedirs(dest, exist_ok=True)
        for name in names:
            assert name.endswith(".gz"), name
            with gzip.open(os.path.join(dirpath, name), "rb") as src, \
                    open(os.path.join(dest, name[:-3]), "wb") as dst:
                dst.write(src.read())
            nfiles += 1
    assert nfiles == 19
    REF = os.path.join(root, "tests")
    DATA = os.path.join(REF, "data")
    return root


def parse_sections(outfile):
    """[(marker_args_str, expected_text), ...] from a .sh.out file."""
    text = open(outfile).read()
    parts = re.split(r"^# dn (.*)$", text, flags=re.M)
    # parts[0] is any preamble; then alternating (args, body)
    sections = []
    for i in range(1, len(parts), 2):
        body = parts[i + 1]
        # the body piece starts with the newline terminating the
        # marker line; histogram sections genuinely begin with a
        # further blank line — strip exactly one
        if body.startswith("\n"):
            body = body[1:]
        sections.append((parts[i], body))
    return sections


def split_args(argstr):
    """The harness echoes `"# dn scan" "$@"`, which flattens the
    quoted JSON filter into space-separated words; re-join a brace-
    balanced run after -f/--filter (the .sh sources single-space the
    JSON, so the reconstruction is exact)."""
    out = []
    i = 0
    n = len(argstr)
    while i < n:
        while i < n and argstr[i] == " ":
            i += 1
        if i >= n:
            break
        if argstr[i] == "{":
            depth = 0
            j = i
            while j < n:
                if argstr[j] == "{":
                    depth += 1
                elif argstr[j] == "}":
                    depth -= 1
                    if depth == 0:
                        j += 1
                        break
                j += 1
            out.append(argstr[i:j])
            i = j
        else:
            j = argstr.find(" ", i)
            if j < 0:
                j = n
            tok = argstr[i:j]
            i = j
            # --filter='{ ... }' flattens into the marker the same
            # way: re-join until braces balance
            if tok.startswith("--filter=") and \
                    tok.count("{") != tok.count("}"):
                while i < n and tok.count("{") != tok.count("}"):
                    j = argstr.find(" ", i + 1)
                    if j < 0:
                        j = n
                    tok += argstr[i:j]
                    i = j
            out.append(tok)
    return out


def sort_d(text):
    """Reproduce the harness's `| sort -d`: dictionary order with
    case folding (the goldens interleave "Aggregator" < {"fields"...}
    < "FindFeedback", i.e. the reference CI's locale folded case;
    -d -f under LC_ALL=C reproduces it deterministically)."""
    r = subprocess.run(["sort", "-d", "-f"], input=text, text=True,
                       capture_output=True,
                       env=dict(os.environ, LC_ALL="C"))
    return r.stdout


def run_section(dn, argstr, datasource="test_file", strip_prefix=None):
    # the harness's scan()/query() append the datasource last:
    # `dn scan "$@" test_file`
    args = split_args(argstr) + [datasource]
    res = dn(*args)
    assert res.code == 0, (argstr, res.err)
    out = res.out
    if strip_prefix:
        out = out.replace(strip_prefix.rstrip("/") + "/", "")
    if args and "--points" in args:
        out = sort_d(out)
    return out


def expected_body(body):
    """A marked section's own output: the harness echoes one blank
    line after each dn invocation."""
    return body.rstrip("\n") + "\n" if body.strip() else ""


def section_own_output(body):
    """Everything up to the blank separator (unmarked trailing output
    from markerless dn invocations is handled by the caller)."""
    return body


def norm(text):
    return text.rstrip("\n") + "\n" if text.strip() else ""


def test_scan_fileset_goldens(dn):
    """tst.scan_fileset.sh.out: the scan_testcases over the whole
    tree (incl. invalid-JSON lines), unmarked gnuplot outputs glued
    to section 25, then dry-run/--counters sections with time-bound
    file pruning (stderr merged by the harness's 2>&1; paths
    sed-stripped to tests/data/...)."""
    sections = parse_sections(
        os.path.join(REF, "dn", "local", "tst.scan_fileset.sh.out"))
    assert len(sections) == 38
    prefix = os.path.dirname(REF.rstrip("/"))  # the unpacked root

    assert dn("datasource-add", "test_input", "--path=" + DATA,
              "--time-format=%Y/%m-%d", "--time-field=time").code == 0
    for argstr, body in sections[:25]:
        got = run_section(dn, argstr, datasource="test_input")
        assert got == expected_body(body), "# dn " + argstr

    # section 25: last scan_testcases section, with the two unmarked
    # `dn scan ... --gnuplot` outputs appended by the harness
    argstr, body = sections[25]
    got = run_section(dn, argstr, datasource="test_input")
    g1 = dn("scan", "-b",
            "timestamp[field=time,date,aggr=lquantize,step=86400]",
            "--gnuplot", "test_input")
    g2 = dn("scan", "-b", "req.method", "--gnuplot", "test_input")
    assert g1.code == 0 and g2.code == 0
    assert norm(got + "\n" + g1.out + g2.out) == norm(body), \
        "# dn " + argstr + " (+gnuplot)"

    # dry-run / counters sections: stdout then stderr (2>&1), paths
    # relative to the workspace root (sed)
    for argstr, body in sections[26:]:
        args = split_args(argstr) + ["test_input"]
        res = dn(*args)
        assert res.code == 0, (argstr, res.err)
        if "--points" in args:
            # `... 2>&1 | sort -d`: sort buffers stdout to EOF, so
            # the unpiped stderr (counters/dry-run list) lands FIRST
            merged = res.err + sort_d(res.out)
        else:
            merged = res.out + res.err
        merged = merged.replace(prefix.rstrip("/") + "/", "")
        assert norm(merged) == norm(body), "# dn " + argstr


def test_empty_goldens(dn, tmp_path):
    """tst.empty.sh.out: /dev/null datasource — empty pretty output
    for breakdowns, the always-one-point zero-breakdown aggregate,
    zero-valued counters omitted, the harness's `2>&1 | sort -d`
    piping BOTH streams through sort, and index build+query over
    EMPTY data (SUM over an empty table yields one row; uncovered
    breakdowns yield none)."""
    sections = parse_sections(
        os.path.join(REF, "dn", "local", "tst.empty.sh.out"))
    scans = [(a, b) for a, b in sections if a.startswith("scan")]
    queries = [(a, b) for a, b in sections if a.startswith("query")]
    assert len(scans) == 12 and len(queries) == 6
    idx = str(tmp_path / "emptyidx")
    assert dn("datasource-add", "devnull", "--path=/dev/null",
              "--index-path=" + idx).code == 0
    for argstr, body in scans:
        args = split_args(argstr) + ["devnull"]
        res = dn(*args)
        assert res.code == 0, (argstr, res.err)
        if "--points" in args:
            merged = sort_d(res.out + res.err)  # 2>&1 INSIDE the pipe
        else:
            merged = res.out + res.err
        assert norm(merged) == norm(body), "# dn " + argstr

    def query(argstr):
        toks = split_args(argstr)
        res = dn(*(["query", "--interval=all"] + toks[1:]
                   + ["devnull"]))
        assert res.code == 0, (argstr, res.err)
        return norm(res.out + res.err)

    assert dn("metric-add", "devnull", "total").code == 0
    assert dn("build", "--interval=all", "devnull").code == 0
    argstr, body = queries[0]
    assert query(argstr) == norm(body), "# dn " + argstr

    assert dn("metric-add", "devnull", "met", "-b",
              "req.method,latency[aggr=quantize]").code == 0
    assert dn("build", "--interval=all", "devnull").code == 0
    for argstr, body in queries[1:]:
        assert query(argstr) == norm(body), "# dn " + argstr


def test_format_skinner_goldens(dn, tmp_path):
    """tst.format_skinner.sh.out: aggregate-of-aggregates — skinner
    points scanned x1/x2/x3 count 250/500/750 (the associativity
    proof), 2-field points re-ground by a coarser breakdown, and a
    build+query round trip over skinner input.  The harness feeds
    /dev/stdin; the replay uses a regular file of identical bytes
    (the char-device read path is covered by the empty-golden
    replay)."""
    sections = parse_sections(
        os.path.join(REF, "dn", "local",
                     "tst.format_skinner.sh.out"))
    assert len(sections) == 5
    one = os.path.join(DATA, "2014", "05-01", "one.log")
    feed = str(tmp_path / "feed.ndjson")

    assert dn("datasource-add", "sk", "--path=" + feed,
              "--data-format=json-skinner").code == 0

    # x1/x2/x3 of the no-field points: 250/500/750
    assert dn("datasource-add", "plain", "--path=" + one).code == 0
    pts = dn("scan", "--points", "plain").out
    for i, (argstr, body) in enumerate(sections[:3]):
        open(feed, "w").write(pts * (i + 1))
        toks = split_args(argstr)
        toks[-1] = "sk"  # the harness's stdin-skinner datasource
        got = dn(*toks)
        assert got.code == 0
        if i == 2:
            # unmarked `dn scan -b req.method stdin` output is glued
            # to this section's body by the harness
            direct = dn("scan", "-b", "req.method", "plain")
            assert norm(got.out + direct.out) == norm(body), argstr
        else:
            assert norm(got.out) == norm(body), argstr

    # x3 of the 2-field points; re-ground by req.method
    pts2 = dn("scan", "--points", "-b", "req.method,res.statusCode",
              "plain").out
    open(feed, "w").write(pts2 * 3)
    argstr, body = sections[3]
    got = dn("scan", "sk")
    assert norm(got.out) == norm(body), argstr

    argstr, body = sections[4]
    got = dn("scan", "sk", "-b", "req.method")
    # the tail glues: "building index" (harness echo to stdout) +
    # `dn query` x2 outputs
    idxdir = str(tmp_path / "idx")
    assert dn("datasource-add", "test_input", "--path=" + feed,
              "--data-format=json-skinner",
              "--index-path=" + idxdir).code == 0
    assert dn("metric-add", "test_input", "total").code == 0
    assert dn("metric-add", "test_input", "-b", "req.method",
              "by_method").code == 0
    b = dn("build", "--interval=all", "test_input")
    assert b.code == 0
    q1 = dn("query", "--interval=all", "test_input")
    q2 = dn("query", "--interval=all", "test_input", "-b",
            "req.method")
    assert q1.code == 0 and q2.code == 0
    combined = (got.out + "building index\n" + b.out
                + q1.out + q2.out)
    assert norm(combined) == norm(body), argstr


def test_index_file_goldens(dn, tmp_path):
    """tst.index_file.sh.out: the scan_testcases answered FROM A
    BUILT INDEX (big 5-column metric incl. a quantized column), then
    a filtered metric, then a datasource-filtered build — all `dn
    query` outputs byte-identical to the reference's golden."""
    sections = parse_sections(
        os.path.join(REF, "dn", "local", "tst.index_file.sh.out"))
    assert len(sections) == 16
    one = os.path.join(DATA, "2014", "05-01", "one.log")
    idx = str(tmp_path / "idx")

    assert dn("datasource-add", "input", "--path=" + one,
              "--index-path=" + idx, "--time-field=time").code == 0
    assert dn("metric-add", "input", "big_metric", "-b",
              "host,operation,req.caller,req.method,"
              "latency[aggr=quantize]").code == 0
    assert dn("build", "input").code == 0
    for argstr, body in sections[:13]:
        got = run_section(dn, argstr, datasource="input")
        assert got == expected_body(body), "# dn " + argstr

    assert dn("metric-remove", "input", "big_metric").code == 0
    assert dn("metric-add", "input", "filtered_metric", "-f",
              '{ "eq": [ "req.method", "GET" ] }').code == 0
    assert dn("build", "input").code == 0
    argstr, body = sections[13]
    got = run_section(dn, argstr, datasource="input")
    assert got == expected_body(body), "# dn " + argstr

    # datasource filter applied at build time
    assert dn("datasource-remove", "input").code == 0
    assert dn("datasource-add", "input", "--path=" + one,
              "--index-path=" + idx, "--time-field=time",
              "--filter", '{ "eq": [ "req.method", "GET" ] }'
              ).code == 0
    assert dn("metric-add", "input", "bycode", "-b",
              "res.statusCode").code == 0
    assert dn("build", "input").code == 0
    for argstr, body in sections[14:]:
        got = run_section(dn, argstr, datasource="input")
        assert got == expected_body(body), "# dn " + argstr


def test_index_fileset_goldens(dn, tmp_path):
    """tst.index_fileset.sh.out: hourly index build over the whole
    tree — the index-tree FILE LISTING must match (layout parity),
    then the scan_testcases answered from the hourly indexes, gnuplot
    output, a filtered metric, and time-bounded query --counters
    (PathEnumerator over the by_hour pattern + Index List / Index
    Result Aggregator stages)."""
    outfile = os.path.join(REF, "dn", "local",
                           "tst.index_fileset.sh.out")
    sections = parse_sections(outfile)
    assert len(sections) == 19
    idx = str(tmp_path / "idx")

    assert dn("datasource-add", "input", "--path=" + DATA,
              "--index-path=" + idx, "--time-field=time",
              "--time-format=%Y/%m-%d").code == 0
    assert dn("metric-add", "input", "myindex", "-b",
              "timestamp[date,field=time,aggr=lquantize,step=86400],"
              "host,operation", "-b",
              "req.caller,req.method,latency[aggr=quantize]"
              ).code == 0
    assert dn("build", "--interval=hour", "input").code == 0

    # the harness lists the built tree: (cd $tmpdir && find . -type f
    # | sort -n) — the listing is the .out preamble
    preamble = open(outfile).read().split("# dn ", 1)[0]
    listing = subprocess.run(
        "find . -type f | sort -n", shell=True, cwd=idx,
        capture_output=True, text=True,
        env=dict(os.environ, LC_ALL="C")).stdout
    assert listing == preamble

    def query(argstr, datasource="input"):
        toks = split_args(argstr)
        assert toks[0] == "query"
        return dn(*(["query", "--interval=hour"] + toks[1:]
                    + [datasource]))

    for argstr, body in sections[:15]:  # testcases + 2 gnuplot
        res = query(argstr)
        assert res.code == 0, (argstr, res.err)
        assert norm(res.out) == norm(body), "# dn " + argstr

    assert dn("metric-remove", "input", "myindex").code == 0
    assert dn("metric-add", "input", "--filter",
              '{ "eq": [ "req.method", "GET" ] }', "-b",
              "timestamp[date,field=time,aggr=lquantize,step=86400]",
              "myindex").code == 0
    assert dn("build", "--interval=hour", "input").code == 0
    argstr, body = sections[15]
    res = query(argstr)
    assert res.code == 0 and norm(res.out) == norm(body), argstr

    assert dn("metric-remove", "input", "myindex").code == 0
    assert dn("metric-add", "input", "myindex", "-b",
              "timestamp[date,field=time,aggr=lquantize,step=60]"
              ).code == 0
    assert dn("build", "--interval=hour", "input").code == 0
    for argstr, body in sections[16:]:
        res = query(argstr)
        assert res.code == 0, (argstr, res.err)
        merged = res.out + res.err  # 2>&1
        assert norm(merged) == norm(body), "# dn " + argstr


def test_config_goldens(dn):
    """tst.config.sh.out: the datasource/metric CRUD surface —
    list/show/update/remove rendering (incl. manta-backend location
    lines), error messages for missing/duplicate entries.  Sections
    whose marker carries an UNTERMINATED JSON filter are skipped:
    their expected text is V8's JSON.parse error wording, which this
    implementation does not reproduce (documented divergence; the
    equivalent failures are covered by our own badargs golden)."""
    sections = parse_sections(
        os.path.join(REF, "dn", "local", "tst.config.sh.out"))
    assert len(sections) == 49
    ran = 0
    for argstr, body in sections:
        if argstr.count("{") != argstr.count("}"):
            continue  # V8 JSON error wording (see docstring)
        args = split_args(argstr)
        res = dn(*args)
        merged = res.out + res.err
        assert norm(merged) == norm(body), "# dn " + argstr
        ran += 1
    assert ran >= 45


def test_badargs_goldens(dn):
    """tst.badargs.sh.out: error wording for malformed breakdowns,
    truncated/unknown-operator filters (node util.inspect predicate
    rendering), --gnuplot arity, and an unsupported data format
    validated at USE time.  The harness pipes through `head -2`, so
    each case pins the first two merged-output lines."""
    one = os.path.join(DATA, "2014", "05-01", "one.log")
    golden = open(os.path.join(
        REF, "dn", "local", "tst.badargs.sh.out")).read().splitlines()
    assert dn("datasource-add", "--path=" + one, "input").code == 0

    cases = [
        ["scan", "-b", "host", "-b", "req.method,x[=bar]", "input"],
        ["scan", "-b", "host", "-b", "req.method,[]", "input"],
        ["scan", "-b", "host", "-b", "req.method,foo[", "input"],
        ["scan", "-f", "{", "input"],
        ["scan", "-f", '{ "junk": [ "foo", "bar" ] }', "input"],
        ["scan", "--gnuplot", "input"],
        ["scan", "-b", "req.method,res.statusCode", "--gnuplot",
         "input"],
    ]
    gi = 0
    for args in cases:
        res = dn(*args)
        assert res.code != 0, args
        mine = (res.out + res.err).splitlines()[:2]
        want = golden[gi:gi + len(mine)]
        assert mine == want, (args, mine, want)
        gi += len(mine)

    # unsupported data format: stored at add time, rejected at scan
    assert dn("datasource-remove", "input").code == 0
    assert dn("datasource-add", "--path=" + one,
              "--data-format=junk", "input").code == 0
    res = dn("scan", "input")
    assert res.code != 0
    assert (res.out + res.err).splitlines()[:1] == golden[gi:gi + 1]


def test_scan_file_goldens(dn):
    """tst.scan_file.sh.out: 26 scan_testcases sections against
    one.log, then 4 sections under a datasource filter
    (reference tests/dn/local/tst.scan_file.sh)."""
    sections = parse_sections(
        os.path.join(REF, "dn", "local", "tst.scan_file.sh.out"))
    assert len(sections) == 30
    one = os.path.join(DATA, "2014", "05-01", "one.log")

    assert dn("datasource-add", "test_file", "--path=" + one).code == 0
    for argstr, body in sections[:26]:
        got = run_section(dn, argstr)
        assert got == expected_body(body), "# dn " + argstr

    assert dn("datasource-remove", "test_file").code == 0
    assert dn("datasource-add", "test_file", "--path=" + one,
              "--filter",
              '{ "eq": [ "req.method", "GET" ] }').code == 0
    for argstr, body in sections[26:]:
        got = run_section(dn, argstr)
        assert got == expected_body(body), "# dn " + argstr


def _worker_manta_replay(rank, world, port, cfgfile, arglists, out_q):
    """One rank of the 2-rank sharded replay of the Manta goldens:
    run every section's scan in lockstep (each scan is collective —
    shard_files + dense RCCL/gloo merge), capturing rank-0 stdout."""
    import io
    import sys as _sys
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    os.environ["LOCAL_RANK"] = str(rank)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["DRAGNET_CONFIG"] = cfgfile
    os.environ["DRAGNET_ENGINE"] = "cpu"
    # CPU ranks: gloo even where a GPU is visible (the default there
    # is RCCL, one device per rank)
    os.environ["DRAGNET_DIST_BACKEND"] = "gloo"
    _sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    from dragnet_amd import cli
    outs = []
    old = _sys.stdout
    for args in arglists:
        buf = io.StringIO()
        _sys.stdout = buf
        try:
            code = cli.main(list(args) + ["testdata"])
        finally:
            _sys.stdout = old
        outs.append((code, buf.getvalue()))
    out_q.put((rank, outs))
    import torch.distributed as dist
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_scan_manta_goldens_sharded(tmp_path):
    """tst.scan_manta.sh.out sections 0-25 (the scan_testcases the
    reference runs through its DISTRIBUTED Manta map/reduce backend)
    replayed byte-for-byte through OUR distributed backend: a 2-rank
    sharded datasource over gloo with the dense tensor merge — the
    strongest distributed-parity evidence we can produce without a
    Manta deployment (reference tests/dn/manta/tst.scan_manta.sh)."""
    import torch.multiprocessing as mp
    sections = parse_sections(
        os.path.join(REF, "dn", "manta", "tst.scan_manta.sh.out"))
    assert len(sections) == 42
    replay = sections[:26]

    cfgfile = str(tmp_path / "rc.json")
    from dragnet_amd import config as mod_config
    cfg = mod_config.DragnetConfig()
    cfg.datasource_add(mod_config.Datasource(
        name="testdata", backend="sharded", path=DATA,
        time_format="%Y/%m-%d", time_field="time"))
    mod_config.save_config(cfg, cfgfile)

    arglists = [split_args(argstr) for argstr, _ in replay]
    ctx = mp.get_context("spawn")
    out_q = ctx.Queue()
    procs = [ctx.Process(target=_worker_manta_replay,
                         args=(r, 2, 29547, cfgfile, arglists, out_q))
             for r in range(2)]
    for p in procs:
        p.daemon = True  # a rank stuck on a dead peer dies with the run
        p.start()
    results = {}
    for _ in range(2):
        rank, outs = out_q.get(timeout=240)
        results[rank] = outs
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0

    for (argstr, body), args, (code, out) in zip(
            replay, arglists, results[0]):
        assert code == 0, argstr
        if "--points" in args:
            out = sort_d(out)
        assert norm(out) == expected_body(body), "# dn " + argstr
    # rank 1 prints nothing
    assert all(code == 0 and out == ""
               for code, out in results[1])


def _worker_index_manta(rank, world, port, cfgfile, idx_root,
                        arglists, out_q):
    """2-rank sharded replay of tst.index_manta.sh: distributed
    builds interleaved with rank-0 config mutations (barriers keep
    the phases in lockstep), queries on every rank (rank 1 prints
    nothing by design)."""
    import io
    import shutil
    import sys as _sys
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    os.environ["LOCAL_RANK"] = str(rank)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["DRAGNET_CONFIG"] = cfgfile
    os.environ["DRAGNET_ENGINE"] = "cpu"
    _sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    from dragnet_amd import cli
    from dragnet_amd.distributed import init_process_group
    dist = init_process_group(backend="gloo")
    old = _sys.stdout

    def run(args):
        buf = io.StringIO()
        _sys.stdout = buf
        try:
            code = cli.main(list(args))
        finally:
            _sys.stdout = old
        return code, buf.getvalue()

    outs = []

    def emit(args):
        outs.append(run(args))

    # phase 1: exhaustive metric, distributed build, 13 queries
    emit(["build", "input"])
    if rank == 0:
        files = []
        for root, _dirs, names in os.walk(idx_root):
            for n in names:
                if n.endswith(".sqlite"):
                    files.append(os.path.relpath(
                        os.path.join(root, n), idx_root))
        outs.append((0, "".join(f + "\n" for f in sorted(files))))
    for args in arglists[:13]:
        emit(list(args) + ["input"])

    # phase 2: filtered index (reference: metric-remove + filtered
    # metric-add + rebuild), then the filtered query
    dist.barrier()
    if rank == 0:
        emit(["metric-remove", "input", "mymet"])
        emit(["metric-add", "input", "-f",
              '{ "eq": [ "req.method", "GET" ] }', "-b",
              "timestamp[date,field=time,aggr=lquantize,step=86400]",
              "mymet"])
    dist.barrier()
    emit(["build", "input"])
    emit(list(arglists[13]) + ["input"])

    # phase 3: datasource filter always applied (mrm -r; update
    # datasource filter; add bycode; rebuild; two queries)
    dist.barrier()
    if rank == 0:
        shutil.rmtree(idx_root)
        emit(["datasource-update", "input",
              '--filter={ "eq": [ "req.method", "GET" ] }'])
        emit(["metric-add", "input", "bycode", "-b",
              "res.statusCode"])
    dist.barrier()
    emit(["build", "input"])
    for args in arglists[14:16]:
        emit(list(args) + ["input"])

    out_q.put((rank, outs))
    dist.barrier()
    import torch.distributed as tdist
    tdist.destroy_process_group()


@pytest.mark.timeout(300)
def test_index_manta_goldens_sharded(tmp_path):
    """tst.index_manta.sh.out replayed through the 2-rank sharded
    backend: partitioned distributed builds (the reference's Manta
    map/reduce build), index file listing, the scan_testcases
    answered from the index, a filtered index, and the
    datasource-filter-always-applied rebuild — byte-for-byte
    (reference tests/dn/manta/tst.index_manta.sh)."""
    import torch.multiprocessing as mp
    text = open(os.path.join(
        REF, "dn", "manta", "tst.index_manta.sh.out")).read()
    parts = re.split(r"^# dn (.*)$", text, flags=re.M)
    preamble = parts[0]
    sections = [(parts[i],
                 parts[i + 1][1:] if parts[i + 1].startswith("\n")
                 else parts[i + 1])
                for i in range(1, len(parts), 2)]
    assert len(sections) == 16

    idx_root = str(tmp_path / "idx")
    cfgfile = str(tmp_path / "rc.json")
    from dragnet_amd import config as mod_config
    cfg = mod_config.DragnetConfig()
    cfg.datasource_add(mod_config.Datasource(
        name="input", backend="sharded", path=DATA,
        time_format="%Y/%m-%d", time_field="time",
        index_path=idx_root))
    cfg.metric_add(mod_config.Metric(
        name="mymet", datasource="input", breakdowns=[
            {"name": "timestamp", "date": "", "field": "time",
             "aggr": "lquantize", "step": 86400},
            {"name": "host"}, {"name": "operation"},
            {"name": "req.caller"}, {"name": "req.method"},
            {"name": "latency", "aggr": "quantize"}]))
    mod_config.save_config(cfg, cfgfile)

    arglists = [["query"] + split_args(a)[1:] for a, _ in sections]
    ctx = mp.get_context("spawn")
    out_q = ctx.Queue()
    procs = [ctx.Process(
        target=_worker_index_manta,
        args=(r, 2, 29549, cfgfile, idx_root, arglists, out_q))
        for r in range(2)]
    for p in procs:
        p.daemon = True  # a rank stuck on a dead peer dies with the run
        p.start()
    results = {}
    for _ in range(2):
        rank, outs = out_q.get(timeout=240)
        results[rank] = outs
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0

    r0 = results[0]
    assert all(code == 0 for code, _ in r0)
    # rank 0's stream: build(no output) + listing + 13 queries +
    # [2 config cmds] + build + query13 + [2 config cmds] + build +
    # queries 14,15
    texts = [out for _code, out in r0]
    assert texts[0] == ""                       # build prints nothing
    assert texts[1] == preamble                 # the mfind listing
    for i in range(13):
        assert norm(texts[2 + i]) == expected_body(sections[i][1]), \
            "# dn " + sections[i][0]
    # config mutations print nothing
    assert texts[15] == texts[16] == ""
    assert texts[17] == ""                      # build 2
    assert norm(texts[18]) == expected_body(sections[13][1])
    assert texts[19] == texts[20] == ""
    assert texts[21] == ""                      # build 3
    assert norm(texts[22]) == expected_body(sections[14][1])
    assert norm(texts[23]) == expected_body(sections[15][1])
    # rank 1 prints nothing anywhere
    assert all(code == 0 and out == "" for code, out in results[1])
