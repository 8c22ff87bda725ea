"""Checks that a split of one file into several is a move.

    python tools/moved_lines.py REV PATH FILE [FILE ...]

PATH as it was at revision REV (`git show REV:PATH`) is compared with the FILEs of the working tree that now hold its text, as
multisets of non-blank lines with trailing whitespace stripped: a line that moved from one file to another, or within one, counts
as found.  Prints the parent's lines that are not found and the new lines the parent did not have, each with its count when it is
more than one; the exit status is 0 either way, the lists are for a reader."""
import collections
import subprocess
import sys


def lines(text):
    return collections.Counter(l.rstrip() for l in text.splitlines() if l.strip())


def report(title, counts):
    print("%s: %d" % (title, sum(counts.values())))
    for line, n in counts.items():
        print("    %s%s" % (line, "" if n == 1 else "    (x%d)" % n))


def main(argv):
    if len(argv) < 4:
        sys.exit(__doc__)
    rev, path, files = argv[1], argv[2], argv[3:]
    old = lines(subprocess.check_output(["git", "show", "%s:%s" % (rev, path)], text=True))
    new = collections.Counter()
    for f in files:
        new += lines(open(f).read())
    print("%s at %s: %d non-blank lines; %s: %d" % (path, rev, sum(old.values()), ", ".join(files), sum(new.values())))
    report("parent lines not found", old - new)
    report("new lines", new - old)


if __name__ == "__main__":
    main(sys.argv)
