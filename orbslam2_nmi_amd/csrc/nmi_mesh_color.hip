// nmi_mesh_color.hip -- the mesh renderer once more, for a mesh with one colour per corner (nmi_render_mesh_colored, coloured mesh
// levels): nmi_mesh_tile_color_kernel and its cover / small forms, the passes in front of them, and launch_render_mesh_colored.
// See the NMI_MESH_COLOR comment at the top of nmi_mesh.hip.
#define NMI_MESH_COLOR 1
#include "nmi_mesh.hip"
