// Stand-alone check of the host side of the station views (nyx_amd/csrc/series_host.h: check_aer_series; nyx_amd/csrc/aer_args.h:
// aer_station_consts, aer_param_needs) - g++ only, no HIP, no GPU (tests/test_aer_host_cxx.py, which builds it with the address and
// undefined-behaviour sanitizers).
//   aer_host_check LAT LON HEIGHT MASK [LAT LON HEIGHT MASK ...]
// runs check_aer_series over a table of cases, then prints, for the stations of the command line (so that nothing is folded at
// compile time: the C library computes them, as in the launcher) on the WGS-84-like ellipsoid of the tests, one line per station:
//   consts r0 r1 r2 s0 s1 s2 e0 e1 e2 z0 z1 z2 mask        (%a: every bit)
// "ok" last.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../nyx_amd/csrc/series_host.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                                              \
    do {                                                                              \
        if (!(cond)) {                                                                \
            if (++g_fail <= 30) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                             \
    } while (0)

static nyx_hip_aer_query_t good_query() {
    nyx_hip_aer_query_t q;
    std::memset(&q, 0, sizeof q);
    q.n_params = 2;
    q.param[0] = NYX_HIP_AER_AZIMUTH;
    q.param[1] = NYX_HIP_AER_RHO_Z;
    q.step_ns = 1000000000LL;
    q.has_frame = 1;
    q.frame_eq_radius_km = 6378.1363;
    q.frame_flattening = 1.0 / 298.257;
    q.frame.kind = NYX_HIP_ROT_IAU;
    q.n_stations = 2;
    q.stations[0] = {40.427222, 4.250556, 0.834939, 5.0};
    q.stations[1] = {-35.398333, 148.981944, 0.691750, 0.0};
    return q;
}

// `why` empty: accepted; else refused with NYX_HIP_RC_BAD_ARG and a message that holds `why`
static void expect(const char *label, const nyx_hip_ctx *ctx, const nyx_hip_traj_t *t, int64_t n, const nyx_hip_aer_query_t *q, int64_t capacity,
                   const double *values, const int32_t *len, const char *why) {
    const Refusal r = check_aer_series(ctx, t, n, q, capacity, values, len);
    if (!*why) {
        CHECK(r.rc == NYX_HIP_RC_OK, "%s: refused with '%s'", label, r.msg);
    } else {
        CHECK(r.rc == NYX_HIP_RC_BAD_ARG && std::strstr(r.msg, why) != nullptr, "%s: rc %d, message '%s', expected '%s'", label, r.rc, r.msg, why);
    }
}

int main(int argc, char **argv) {
    // ---- the refusals, in the order the checks fire
    const nyx_hip_ctx *ctx = (const nyx_hip_ctx *)(uintptr_t)1;   // never dereferenced
    int64_t epoch[1] = {0};
    double x[1] = {0};
    int32_t tl[1] = {0};
    nyx_hip_traj_t t;
    std::memset(&t, 0, sizeof t);
    t.capacity = 1;
    t.epoch_ns = epoch;
    t.x_km = t.y_km = t.z_km = t.vx_km_s = t.vy_km_s = t.vz_km_s = x;
    t.len = tl;
    double values[1];
    int32_t len[1];
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    nyx_hip_aer_query_t q = good_query();
    expect("good", ctx, &t, 1, &q, 4, values, len, "");
    expect("n = 0", ctx, &t, 0, &q, 4, values, len, "");
    expect("null ctx", nullptr, &t, 1, &q, 4, values, len, "null ctx");
    nyx_hip_traj_t bad_t = t;
    bad_t.len = nullptr;
    expect("null array", ctx, &bad_t, 1, &q, 4, values, len, "traj: null array");
    expect("null query", ctx, &t, 1, nullptr, 4, values, len, "traj_aer: null query");
    expect("negative n", ctx, &t, -1, &q, 4, values, len, "negative n");
#define CASE(label, mutate, cap, why) do { q = good_query(); mutate; expect(label, ctx, &t, 1, &q, cap, values, len, why); } while (0)
    CASE("no parameter", q.n_params = 0, 4, "n_params = 0, 1 .. 8");
    CASE("nine parameters", q.n_params = 9, 4, "n_params = 9, 1 .. 8");
    CASE("unknown parameter", q.param[1] = NYX_HIP_AER_COUNT, 4, "param[1] = 9 is not a nyx_hip_aer_param");
    CASE("negative parameter", q.param[0] = -1, 4, "param[0] = -1");
    CASE("step 0", q.step_ns = 0, 4, "step_ns must be > 0");
    CASE("capacity 0", (void)0, 0, "capacity must be 1 .. 2^31 - 1");
    CASE("capacity 2^31", (void)0, (int64_t)INT32_MAX + 1, "capacity must be 1 .. 2^31 - 1");
    CASE("no station", q.n_stations = 0, 4, "n_stations = 0, 1 .. 16");
    CASE("seventeen stations", q.n_stations = 17, 4, "n_stations = 17, 1 .. 16");
    CASE("sixteen stations", q.n_stations = 16, 4, "");   // (the rest of the table is zeros: stations on the equator)
    CASE("latitude 90.5", q.stations[1].latitude_deg = 90.5, 4, "stations[1].latitude_deg");
    CASE("latitude -91", q.stations[0].latitude_deg = -91.0, 4, "stations[0].latitude_deg");
    CASE("latitude NaN", q.stations[0].latitude_deg = nan, 4, "stations[0].latitude_deg");
    CASE("latitude 90", q.stations[0].latitude_deg = 90.0, 4, "");
    CASE("longitude inf", q.stations[1].longitude_deg = inf, 4, "stations[1].longitude_deg");
    CASE("longitude NaN", q.stations[0].longitude_deg = nan, 4, "stations[0].longitude_deg");
    CASE("longitude 725", q.stations[0].longitude_deg = 725.0, 4, "");
    CASE("height -inf", q.stations[1].height_km = -inf, 4, "stations[1].height_km");
    CASE("mask 91", q.stations[1].elevation_mask_deg = 91.0, 4, "stations[1].elevation_mask_deg");
    CASE("mask NaN", q.stations[0].elevation_mask_deg = nan, 4, "stations[0].elevation_mask_deg");
    CASE("a bad station beyond n_stations is not read", q.stations[2].latitude_deg = 200.0, 4, "");
    CASE("Euler-Chebyshev frame", q.frame.kind = NYX_HIP_ROT_EULER_CHEBY, 4, "NYX_HIP_ROT_IAU");
    CASE("n_nut_prec -1", q.frame.n_nut_prec = -1, 4, "n_nut_prec = -1");
    CASE("n_nut_prec 17", q.frame.n_nut_prec = NYX_HIP_MAX_NUT_PREC + 1, 4, "n_nut_prec = 17");
    CASE("radius 0", q.frame_eq_radius_km = 0.0, 4, "frame_eq_radius_km must be > 0");
    CASE("radius NaN", q.frame_eq_radius_km = nan, 4, "frame_eq_radius_km must be > 0");
    CASE("flattening 1", q.frame_flattening = 1.0, 4, "frame_flattening");
    CASE("flattening < 0", q.frame_flattening = -1e-3, 4, "frame_flattening");
    // which check wins: the parameters before the step, the step before the stations, the stations before the frame
    CASE("parameters before step", (q.n_params = 0, q.step_ns = 0), 4, "n_params");
    CASE("step before stations", (q.step_ns = 0, q.n_stations = 0), 4, "step_ns");
    CASE("stations before frame", (q.n_stations = 0, q.frame.kind = NYX_HIP_ROT_EULER_CHEBY), 4, "n_stations");
    CASE("frame before outputs", q.frame_flattening = 1.0, 4, "frame_flattening");
    q = good_query();
    expect("null values", ctx, &t, 1, &q, 4, nullptr, len, "values and len arrays required");
    expect("null len", ctx, &t, 1, &q, 4, values, nullptr, "values and len arrays required");

    // ---- what each parameter needs
    CHECK(aer_param_needs(NYX_HIP_AER_AZIMUTH) == AER_NEED_AZIMUTH && aer_param_needs(NYX_HIP_AER_RANGE_RATE) == AER_NEED_RANGE_RATE, "needs");
    CHECK(aer_param_needs(NYX_HIP_AER_ELEVATION) == AER_NEED_ELEVATION && aer_param_needs(NYX_HIP_AER_ELEVATION_ABOVE_MASK) == AER_NEED_ELEVATION &&
              aer_param_needs(NYX_HIP_AER_VISIBLE) == AER_NEED_ELEVATION, "needs");
    CHECK(aer_param_needs(NYX_HIP_AER_RANGE) == 0 && aer_param_needs(NYX_HIP_AER_RHO_S) == 0 && aer_param_needs(NYX_HIP_AER_RHO_E) == 0 &&
              aer_param_needs(NYX_HIP_AER_RHO_Z) == 0, "needs");
    CHECK(aer_param_needs(NYX_HIP_AER_COUNT) == -1 && aer_param_needs(-1) == -1, "needs");

    // ---- the constants of the stations of the command line, sixteen per query
    const int n_st = (argc - 1) / 4;
    CHECK((argc - 1) % 4 == 0, "four numbers per station");
    for (int s0 = 0; s0 < n_st; s0 += NYX_HIP_MAX_STATIONS) {
        q = good_query();
        q.n_stations = n_st - s0 < NYX_HIP_MAX_STATIONS ? n_st - s0 : NYX_HIP_MAX_STATIONS;
        for (int s = 0; s < q.n_stations; ++s) {
            char **a = argv + 1 + 4 * (s0 + s);
            q.stations[s] = {std::strtod(a[0], nullptr), std::strtod(a[1], nullptr), std::strtod(a[2], nullptr), std::strtod(a[3], nullptr)};
        }
        AerStationConsts c[NYX_HIP_MAX_STATIONS];
        aer_station_consts(q, c);
        for (int s = 0; s < q.n_stations; ++s) {
            std::printf("consts");
            for (const double *v : {c[s].r_km, c[s].south, c[s].east, c[s].zenith})
                for (int k = 0; k < 3; ++k) std::printf(" %a", v[k]);
            std::printf(" %a\n", c[s].mask_deg);
            // a right-handed orthonormal triad, the station on its own zenith line within rounding
            const double *S = c[s].south, *E = c[s].east, *Z = c[s].zenith;
            const double x[3] = {S[1] * E[2] - S[2] * E[1], S[2] * E[0] - S[0] * E[2], S[0] * E[1] - S[1] * E[0]};
            CHECK(std::fabs(x[0] - Z[0]) < 1e-15 && std::fabs(x[1] - Z[1]) < 1e-15 && std::fabs(x[2] - Z[2]) < 1e-15, "station %d: S x E != Z", s0 + s);
        }
    }
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("ok\n");
    return 0;
}
