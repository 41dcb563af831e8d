"""
Add or refresh the columnar sidecars of an existing index tree:

    python -m dragnet_amd.tools.index_columnar [--force] INDEX_ROOT

Every index file under INDEX_ROOT (the `all` file, `by_day/*.sqlite`,
`by_hour/*.sqlite`) gets a `.dncol` sidecar beside it
(dragnet_amd/index/columnar.py).  A sidecar that is fresh and passes
every check is left alone, so a second run writes nothing; --force
rewrites them all.  Prints one line per file: "wrote" or "fresh".
"""

import os
import sys

from ..index import columnar


def index_files(root):
    """The index files of a tree, sorted: the interval-less `all` file
    and every *.sqlite below the root."""
    out = []
    for d, _dirs, names in os.walk(root):
        for n in names:
            if n.endswith(".sqlite") or (n == "all" and d == root):
                out.append(os.path.join(d, n))
    return sorted(out)


def refresh(root, force=False, out=None):
    """-> (number written, number left alone)."""
    nwrote = nfresh = 0
    for path in index_files(root):
        if not force and columnar.open_sidecar(path, full=True) is not None:
            nfresh += 1
            verdict = "fresh"
        else:
            columnar.write_sidecar(path)
            nwrote += 1
            verdict = "wrote"
        if out is not None:
            out.write("%s %s\n" % (verdict, columnar.sidecar_path(path)))
    return nwrote, nfresh


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    force = "--force" in argv
    args = [a for a in argv if a != "--force"]
    if len(args) != 1 or args[0].startswith("-"):
        sys.stderr.write(
            "usage: python -m dragnet_amd.tools.index_columnar "
            "[--force] INDEX_ROOT\n")
        return 2
    if not os.path.isdir(args[0]):
        sys.stderr.write("index_columnar: not a directory: %s\n" % args[0])
        return 1
    refresh(args[0], force=force, out=sys.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
