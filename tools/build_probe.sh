# Timing-probe variants of the library: builds tools/probe_lib/libgnss_probe<N>.so for each
# N given, with GNSS_CORR_PROBE=N (track.hip: bits that drop parts of the correlator; 0 =
# the full correlator) and GNSS_PROBE_BUILD=1 (the api_*.cpp host files read the GNSS_STAMPS /
# GNSS_PROBE / GNSS_HOSTPROF / GNSS_FORCE_SUB10 environment hooks). Load one with
# GNSS_LIB=<path>. Never used by the product, the tests or bench.py. EXTRA_FLAGS adds
# compiler flags.
set -e
cd "$(dirname "$0")/../assignment-for-aae6102_gnss-sdr_amd/csrc"
make -s
mkdir -p ../../tools/probe_lib /tmp/gnss_probe_obj
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -pthread -DGNSS_PROBE_BUILD=1 $EXTRA_FLAGS"
HOST=$(grep -l "probe_env(" *.cpp | sed "s/\.cpp$//")  # the host files that call probe_env
for h in $HOST; do
  /opt/rocm/bin/hipcc $FLAGS -c $h.cpp -o /tmp/gnss_probe_obj/${h}_host.o &
done
for n in "$@"; do
  /opt/rocm/bin/hipcc $FLAGS -DGNSS_CORR_PROBE=$n -c track.hip -o /tmp/gnss_probe_obj/track_$n.o &
done
wait
for n in "$@"; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../tools/probe_lib/libgnss_probe$n.so \
    /tmp/gnss_probe_obj/track_$n.o $(for h in $HOST; do echo /tmp/gnss_probe_obj/${h}_host.o; done) \
    $(make -s print-objs | tr ' ' '\n' | grep -v -e '/track.o$' $(for h in $HOST; do echo "-e /${h}_host.o\$"; done)) \
    -L/opt/rocm/lib -lrocfft -pthread -Wl,-rpath,/opt/rocm/lib
done
ls -la ../../tools/probe_lib
