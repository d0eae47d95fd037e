// nmi_map_color.cpp -- OBJ meshes with one colour per vertex ("v x y z r g b", the extension MeshLab, CloudCompare and Open3D
// write for reconstructions without a texture atlas), read into the per-corner arrays of nmi_render_mesh_colored.  Declared in
// include/nmi_host.h; host only.  The reference has no loader for such a file (its loadOBJ, objloader.cpp:140-224, takes "v x y z"
// and needs a "vt" per corner); the grammar outside the vertex and face lines is nmi_map_load_obj's: any other first word drops
// its line.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>

#include "nmi_host.h"

namespace {

template <typename T>
T *take(const std::vector<T> &v)
{
    T *p = static_cast<T *>(malloc(v.empty() ? sizeof(T) : v.size() * sizeof(T)));
    if (p && !v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

struct File {
    FILE *f;
    explicit File(const char *path, const char *mode) : f(path ? fopen(path, mode) : nullptr) {}
    ~File()
    {
        if (f) fclose(f);
    }
};

// One face corner, "a", "a/b", "a//c" or "a/b/c": the position index a (1-based); b and c only have to be numbers.
bool corner_index(const char *word, unsigned long *a)
{
    char *end = nullptr;
    if (*word < '0' || *word > '9') return false;
    *a = strtoul(word, &end, 10);
    for (int part = 0; part < 2 && *end == '/'; ++part) {
        const char *p = end + 1;
        if (part == 0 && *p == '/') {  // "a//c"
            end = const_cast<char *>(p);
            continue;
        }
        if (*p < '0' || *p > '9') return false;
        (void)strtoul(p, &end, 10);
    }
    return *end == '\0';
}

}  // namespace

extern "C" {

// "v x y z r g b": colours are floats in [0, 1] and are taken as they are (no 1/256 as for loadXYZ's byte colours).  "f" with three
// corners in any of the four index forms; every corner becomes one vertex of the output, in file order, as in nmi_map_load_obj.
// -2: a vertex line with fewer than six numbers (no colours), a face that is not three corners; -3: a position index outside the
// file's vertex list; -5: the file cannot be opened; -6: out of memory.  `red` [n] is the r column -- what the render's GL_RED
// target keeps -- and `rgb` [n][3] (optional) the whole colour.
int nmi_map_load_obj_colored(const char *path, float **xyz, float **red, float **rgb, int64_t *n_vertices)
{
    if (!path || !xyz || !red || !n_vertices) return -1;
    *xyz = nullptr, *red = nullptr, *n_vertices = 0;
    if (rgb) *rgb = nullptr;
    File in(path, "r");
    if (!in.f) return -5;
    try {
        std::vector<float> pos, col;
        std::vector<unsigned long> ipos;
        char line[1024];
        while (fgets(line, sizeof line, in.f)) {
            if (!strchr(line, '\n') && !feof(in.f)) {  // a longer line: its first 1023 characters decide, the rest is dropped
                int c;
                while ((c = fgetc(in.f)) != EOF && c != '\n') {}
            }
            char word[8];
            int at = 0;
            if (sscanf(line, "%7s%n", word, &at) != 1) continue;  // blank
            if (strcmp(word, "v") == 0) {
                float v[6];
                if (sscanf(line + at, "%f %f %f %f %f %f", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) != 6) return -2;
                pos.insert(pos.end(), v, v + 3);
                col.insert(col.end(), v + 3, v + 6);
            } else if (strcmp(word, "f") == 0) {
                char c[4][64];
                if (sscanf(line + at, "%63s %63s %63s %63s", c[0], c[1], c[2], c[3]) != 3) return -2;  // triangles only
                for (int k = 0; k < 3; ++k) {
                    unsigned long a = 0;
                    if (!corner_index(c[k], &a)) return -2;
                    ipos.push_back(a);
                }
            }
            // any other keyword (comments, vt, vn, usemtl, s, g ...): the line is dropped
        }
        std::vector<float> out_xyz, out_red, out_rgb;
        out_xyz.reserve(ipos.size() * 3), out_red.reserve(ipos.size());
        if (rgb) out_rgb.reserve(ipos.size() * 3);
        for (size_t i = 0; i < ipos.size(); ++i) {
            if (ipos[i] < 1 || ipos[i] > pos.size() / 3) return -3;
            const size_t at = (size_t)(ipos[i] - 1) * 3;
            out_xyz.insert(out_xyz.end(), pos.begin() + at, pos.begin() + at + 3);
            out_red.push_back(col[at]);
            if (rgb) out_rgb.insert(out_rgb.end(), col.begin() + at, col.begin() + at + 3);
        }
        *xyz = take(out_xyz), *red = take(out_red);
        if (rgb) *rgb = take(out_rgb);
        if (!*xyz || !*red || (rgb && !*rgb)) {
            free(*xyz), free(*red);
            *xyz = nullptr, *red = nullptr;
            if (rgb) free(*rgb), *rgb = nullptr;
            return -6;
        }
        *n_vertices = (int64_t)ipos.size();
    } catch (const std::bad_alloc &) {
        return -6;
    }
    return 0;
}

}  // extern "C"
