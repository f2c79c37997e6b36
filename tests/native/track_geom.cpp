// The tracking steps' lane geometry (csrc/track_geom.h: what api_track.cpp's tracking_impl and
// gnss_correlate_step call) on the CPU. argv[1]: a table written by the pytest function from
// tests/rate_matrix.py's independent restatement, one case per line
//   Fs Sample pdi forced sub bpc
// (int8 records, 3 taps, k/Fs by reciprocal). Then the rules the table does not reach: the
// int16 / 25-tap spans, overrides the rule rejects, and the virtual-block search.
#include <cstdio>
#include <cstdlib>

#include "../../assignment-for-aae6102_gnss-sdr_amd/csrc/track_geom.h"

using namespace gnss::geom;

static int bad = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            bad++;                                                    \
            printf("line %d: %s\n", __LINE__, #cond);                 \
        }                                                             \
    } while (0)

static const double kFc = 1.023e6;
static LaneRule rule(double Fs, int fmt, int ntaps, bool exact_div) { return LaneRule{1.1 * kFc / Fs, fmt, ntaps, exact_div}; }

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* fp = fopen(argv[1], "r");
    if (!fp) return 2;
    double Fs;
    long long S;
    int pdi, forced, sub, bpc, rows = 0;
    while (fscanf(fp, "%lf %lld %d %d %d %d", &Fs, &S, &pdi, &forced, &sub, &bpc) == 6) {
        rows++;
        for (int ntaps : {3, 11}) {
            const LaneRule r = rule(Fs, 0, ntaps, false);
            const int s = sub_override(r, sub_for(r, pdi), 0, forced);
            const int b = bpc_for(S, pdi, s);
            if (s != sub || b != bpc) {
                bad++;
                printf("Fs %.17g pdi %d forced %d taps %d: (%d, %d), expected (%d, %d)\n", Fs, pdi, forced, ntaps, s, b,
                       sub, bpc);
            }
        }
    }
    fclose(fp);
    CHECK(rows >= 12);

    // int16 records and 25 taps: 8- or 24-sample lanes only
    for (double fs : {58e6, 26e6, 16.3676e6, 12.5e6, 10e6, 8.5e6})
        for (int form = 0; form < 2; form++) {
            const LaneRule r = rule(fs, form == 0 ? 1 : 0, form == 0 ? 3 : 25, false);
            for (int p : {1, 10}) {
                const int own = sub_for(r, p);
                CHECK(own == 1 || own == 3);
                CHECK(p == 10 || own == 1);
                CHECK(own != 3 || sub_ok(r, 3));
                for (int v = 0; v <= 5; v++) {
                    const int f = sub_override(r, own, 0, v);
                    CHECK(f == 1 || f == 3);
                    CHECK(f == own || (f == v && sub_ok(r, v)));
                    CHECK(sub_override(r, own, v, 0) == own);  // (the probe hook: int8 below 25 taps only)
                }
            }
        }
    CHECK(sub_for(rule(58e6, 1, 3, false), 10) == 3 && sub_for(rule(58e6, 0, 25, false), 10) == 3);
    CHECK(sub_for(rule(26e6, 1, 3, false), 10) == 1);  // (16-sample lanes are not an int16 form)
    CHECK(sub_for(rule(26e6, 0, 3, false), 10) == 2);

    // an override the rule rejects is ignored
    {
        const LaneRule r26 = rule(26e6, 0, 3, false), r58 = rule(58e6, 0, 3, false), rdiv = rule(58e6, 0, 3, true);
        CHECK(!sub_ok(r26, 3) && sub_override(r26, 2, 0, 3) == 2 && sub_override(r26, 2, 3, 0) == 2);
        CHECK(!sub_ok(r26, 4) && sub_override(r26, 1, 0, 4) == 1);
        CHECK(sub_override(r58, 3, 0, 4) == 4 && sub_override(r58, 1, 2, 0) == 2);
        CHECK(sub_override(r58, 1, 2, 4) == 4);  // (the test hook after the probe hook)
        CHECK(sub_override(r58, 3, 0, 5) == 3 && sub_override(r58, 3, 0, -1) == 3 && sub_override(r58, 3, 7, 0) == 3);
        // k/Fs by division: 8-sample lanes only
        CHECK(sub_for(rdiv, 10) == 1 && sub_override(rdiv, 1, 0, 3) == 1 && sub_override(rdiv, 1, 0, 1) == 1);
        const LaneRule low = rule(8.5e6, 0, 3, false);  // inside the margin: sub_ok(1) is false, the span stays 1
        CHECK(!sub_ok(low, 1) && sub_for(low, 1) == 1 && sub_for(low, 10) == 1 && sub_override(low, 1, 0, 2) == 1);
    }

    // the virtual-block search
    {
        int asked_v = 0;
        auto occ = [](int v) { return [v] { return v; }; };
        auto occv = [&](int v) {
            return [&asked_v, v] {
                asked_v++;
                return v;
            };
        };
        const int bpc10 = bpc_for(58000, 10, 3);
        CHECK(bpc10 == 96 && bpc_for(58000, 1, 1) == 29);
        // 8 x 96 blocks at 3 per CU on 256 CUs: all resident, the virtual form is not asked about
        CHECK(vpb_for(false, 8, 96, 256, 0, occ(3), occv(3)) == 1 && asked_v == 0);
        CHECK(vpb_for(false, 8, 96, 256, 0, occ(2), occv(0)) == 0 && asked_v == 1);  // (no virtual form)
        CHECK(vpb_for(false, 8, 97, 256, 0, occ(3), occv(3)) == 2);
        // config 5: 32 channels x 11 taps at 2 blocks per CU
        const int v5 = vpb_for(false, 32, bpc10, 256, 0, occ(2), occ(2));
        CHECK(v5 > 1 && 32 * ((bpc10 + v5 - 1) / v5) <= 2 * 256 && 32 * ((bpc10 + v5 - 2) / (v5 - 1)) > 2 * 256);
        CHECK(vpb_for(false, 32, bpc10, 256, 0, occ(9), occ(9)) == 3);  // (occupancy counted up to 4 per CU)
        CHECK(vpb_for(true, 8, 96, 256, 0, occ(3), occ(3)) == 0);       // no_persist
        CHECK(vpb_for(true, 8, 96, 256, 5, occ(3), occ(3)) == 0);
        CHECK(vpb_for(false, 8, 96, 256, 5, occ(3), occ(3)) == 5);      // GNSS_OPT_FORCE_VPB: at least that many
        CHECK(vpb_for(false, 8, 96, 256, 1000, occ(3), occ(3)) == kVpbMax);
        CHECK(vpb_for(false, 8, 96, 256, 1, occ(3), occ(3)) == 1);
        CHECK(vpb_for(false, 1000, 96, 256, 0, occ(4), occ(4)) == 0);   // fits at no vpb
        CHECK(vpb_for(false, 8, 96, 256, 0, occ(0), occ(0)) == 0);
    }
    printf("cases %d, mismatches %d\n", rows, bad);
    return bad ? 1 : 0;
}
