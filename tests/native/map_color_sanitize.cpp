// ASan/UBSan exercise of nmi_map_load_obj_colored (host/nmi_map_color.cpp, no GPU): a well-formed file, truncations of it,
// random byte corruption, over-long lines and words, huge and negative indices.  Every call must return cleanly, with its outputs
// released or null.  Built and run by tests/test_mesh_color.py with -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "nmi_host.h"

static unsigned rng_state = 2468u;
static unsigned rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

static std::string path_in_tmp(const char *name)
{
    const char *t = getenv("TMPDIR");
    return std::string(t && *t ? t : "/tmp") + "/" + name;
}

// Writes `text`, loads it, releases what came back.  -> the loader's code; on failure the outputs must be null.
static int load(const std::string &text, int64_t *n_out = nullptr, float *first_red = nullptr)
{
    const std::string p = path_in_tmp("map_color_sanitize.obj");
    FILE *f = fopen(p.c_str(), "wb");
    if (!f) exit(90);
    fwrite(text.data(), 1, text.size(), f);
    fclose(f);
    float *xyz = (float *)1, *red = (float *)1, *rgb = (float *)1;
    int64_t n = -1;
    const int rc = nmi_map_load_obj_colored(p.c_str(), &xyz, &red, &rgb, &n);
    if (rc != 0 && (xyz || red || rgb || n != 0)) exit(91);
    if (rc == 0) {
        float sum = 0.0f;  // touch every element: a short buffer shows under ASan
        for (int64_t i = 0; i < n; ++i) sum += xyz[i * 3] + xyz[i * 3 + 1] + xyz[i * 3 + 2] + red[i] + rgb[i * 3] + rgb[i * 3 + 1] + rgb[i * 3 + 2];
        if (first_red && n > 0) *first_red = red[0] + 0.0f * sum;
    }
    if (n_out) *n_out = n;
    nmi_map_free(xyz), nmi_map_free(red), nmi_map_free(rgb);
    return rc;
}

int main()
{
    const std::string good =
        "# quad\nv 0 0 0 1 0 0\nv 1 0 0 0 1 0\nvt 0.5 0.5\nv 1 1 0 0.25 0.5 0.75\nvn 0 0 1\nv 0 1 0.5 0.125 1 0\n"
        "f 1 2 3\nf 1/1 3/1 4/1\nf 4//1 3//1 2//1\nf 2/1/1 1/1/1 4/1/1\n";
    int64_t n = 0;
    float r0 = 0.0f;
    if (load(good, &n, &r0) != 0 || n != 12 || r0 != 1.0f) return 1;
    for (size_t cut = 0; cut <= good.size(); cut += 7) (void)load(good.substr(0, cut));  // truncations: inside words, numbers and lines
    for (int it = 0; it < 150; ++it) {                                                    // random byte corruption
        std::string s(good);
        for (int k = 0; k < 1 + (int)(rnd() % 6); ++k) s[rnd() % s.size()] = (char)(rnd() & 0xFF);
        (void)load(s);
    }
    if (load(good + "f 1 2 5\n") != -3 || load(good + "f 0 1 2\n") != -3) return 2;
    if (load(good + "f 1 2 99999999999999999999999999\n") != -3) return 3;              // saturates, still out of range
    if (load(good + "f -1 -2 -3\n") != -2 || load(good + "f 1 2\n") != -2 || load(good + "f 1 2 3 4\n") != -2) return 4;
    if (load(good + "f 1/ 2 3\n") != -2 || load(good + "f 1/2/3/4 2 3\n") != -2 || load(good + "f 1x 2 3\n") != -2) return 5;
    if (load("v 1 2 3\nf 1 1 1\n") != -2 || load("v 1 2 3 0.5 0.5\n") != -2) return 6;                           // no (whole) colour
    if (load(good + "f " + std::string(5000, '1') + " 2 3\n") != -2) return 7;          // a corner longer than any index
    if (load(good + "# " + std::string(5000, 'c') + " v 1 2 3\nf 1 2 3\n", &n) != 0 || n != 15) return 8;       // an over-long comment is ONE line
    if (load(good + std::string(3000, 'k') + " 1 2 3\n", &n) != 0 || n != 12) return 9;  // an over-long keyword is no keyword
    if (load("", &n) != 0 || n != 0) return 10;
    float *x = nullptr, *r = nullptr;
    if (nmi_map_load_obj_colored(path_in_tmp("no_such_file.obj").c_str(), &x, &r, nullptr, &n) != -5 || x || r) return 11;
    if (nmi_map_load_obj_colored(nullptr, &x, &r, nullptr, &n) != -1 || nmi_map_load_obj_colored("x", nullptr, &r, nullptr, &n) != -1) return 12;
    printf("map color sanitize ok\n");
    return 0;
}
