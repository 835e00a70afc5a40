#!/usr/bin/env bash
# Build the reference encoder WITH the N1 patch against this repository's C ABI.
#
# Build container only: needs /root/reference/vtm-mlt-cpp (the authors' VTM-11.0 tree).  Nothing of the reference enters
# the repository: the tree is copied to a scratch directory, patches/vtm-mlt-cpp-mltcnn.patch is applied with zero fuzz,
# and the reference's OWN CMake project is configured with -DMLTCNN_ROOT=<this repository> (after the patch it needs
# neither LibTorch nor OpenCV).  Products (EncoderApp / DecoderApp binaries) are copied to <repo>/oracle/_ref/vtm/, which is
# git-ignored but travels to the GPU box with the snapshot.
#
#   tools/build_vtm.sh [--ref DIR] [--work DIR] [--jobs N]
#
# The binaries are TEST binaries: host/mlt_split_predictor.hpp is compiled with -DMLTCNN_TEST_HOOKS (fault injection + call dump; a production
# build of the patched encoder carries neither).
# The anchor (stock VTM-11.0 RDO) needs no second build: MLTCNN_SIZE_MASK=0x100 enables no CU size, so gate() is false
# for every CU (tests/test_vtm_encoder.py compares its bitstream with the failure-injected and the no-device runs).
#
# gcc 11 finds -Wmaybe-uninitialized / -Wstringop-overflow style diagnostics in stock VTM-11.0 that its -Werror turns
# into errors; they are demoted to warnings here (more specific -Wno-error=... wins over -Werror regardless of order).
set -euo pipefail
REPO="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
REF=/root/reference/vtm-mlt-cpp
# one scratch tree per user and checkout: another user's tree is not writable, another checkout's would configure against its own repository
WORK=${TMPDIR:-/tmp}/mltcnn_vtm-$(id -u)-$(printf '%s' "$REPO" | sha256sum | cut -c1-12)
JOBS=6
while [ $# -gt 0 ]; do
  case "$1" in
    --ref) REF="$2"; shift 2;;
    --work) WORK="$2"; shift 2;;
    --jobs) JOBS="$2"; shift 2;;
    *) echo "unknown argument $1" >&2; exit 2;;
  esac
done
[ -d "$REF/source/Lib/EncoderLib" ] || { echo "reference tree not found at $REF" >&2; exit 3; }
[ -f "$REPO/fastintercu-vvc_amd/libmltcnn_hip.so" ] || (cd "$REPO" && python -c "import __graft_entry__ as g; g.build()")

mkdir -p "$WORK"
# N1 (the call-site replacement) and, on top of it, the opt-in N3 patch (encoder-side batching: probe and replay over WPP anti-diagonals;
# dormant unless MLTCNN_BATCH=1 -- without it the binary runs the N1 code path).  The scratch tree is re-made when either patch changed.
PATCHSUM=$(cat "$REPO/patches/vtm-mlt-cpp-mltcnn.patch" "$REPO/patches/vtm-mlt-cpp-mltcnn-n3.patch" | sha256sum | cut -c1-16)
if [ ! -f "$WORK/src/.patched" ] || [ "$(cat "$WORK/src/.patched")" != "$PATCHSUM" ]; then
  rm -rf "$WORK/src"; mkdir -p "$WORK/src"
  (cd "$REF" && cp -r CMakeLists.txt cmake source cfg "$WORK/src/")
  chmod -R u+w "$WORK/src"   # the copy keeps the reference's read-only modes: patch and CMake write into it
  (cd "$WORK/src" && patch -p1 --fuzz=0 < "$REPO/patches/vtm-mlt-cpp-mltcnn.patch")
  (cd "$WORK/src" && patch -p1 --fuzz=0 < "$REPO/patches/vtm-mlt-cpp-mltcnn-n3.patch")
  echo "$PATCHSUM" > "$WORK/src/.patched"
fi

WNO="-Wno-error=maybe-uninitialized -Wno-error=stringop-overflow -Wno-error=array-bounds -Wno-error=uninitialized -Wno-error=deprecated-declarations -Wno-error=unused-but-set-variable -Wno-error=address -Wno-error=nonnull -Wno-error=restrict -Wno-error=stringop-truncation -Wno-error=format-truncation -Wno-error=misleading-indentation"
build_one() {  # $1 = build dir name, $2 = extra CXX flags, $3 = output suffix
  mkdir -p "$WORK/$1"
  (cd "$WORK/$1" && cmake "$WORK/src" -DCMAKE_BUILD_TYPE=Release -DMLTCNN_ROOT="$REPO" -DCMAKE_CXX_FLAGS="$WNO -DMLTCNN_TEST_HOOKS $2" > cmake.log 2>&1) || { tail -20 "$WORK/$1/cmake.log"; exit 4; }
  (cd "$WORK/$1" && make -j"$JOBS" EncoderApp DecoderApp > make.log 2>&1) || { grep -n "error" "$WORK/$1/make.log" | head -20; exit 5; }
  mkdir -p "$REPO/oracle/_ref/vtm"
  # the reference's CMake writes binaries to <src>/bin (BBuildEnv); pick up the freshest EncoderApp / DecoderApp
  for app in EncoderApp DecoderApp; do
    f=$(find "$WORK/src/bin" "$WORK/$1" -type f -name "${app}" -perm -u+x -printf '%T@ %p\n' 2>/dev/null | sort -rn | head -1 | cut -d' ' -f2-)
    [ -n "$f" ] || { echo "$app not found after the build" >&2; exit 6; }
    cp "$f" "$REPO/oracle/_ref/vtm/${app}$3"
  done
}
build_one build "" ""
ls -la "$REPO/oracle/_ref/vtm"
