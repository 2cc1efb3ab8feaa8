#!/bin/bash
# build git revision $1 (default HEAD) with that revision's own iqlpref_amd/build.py, from an export in a
# temp directory, as iqlpref_amd/libiqlhip_prev.so for tools/ab.sh.  Run from the repository root.
set -e
REV=${1:-HEAD}
D=$(mktemp -d)
trap 'rm -rf "$D"' EXIT
git archive "$REV" | tar -x -C "$D"
(cd "$D" && python -m iqlpref_amd.build --force)
cp "$D/iqlpref_amd/libiqlhip.so" iqlpref_amd/libiqlhip_prev.so
