/* clean_cmd.c -- `fermi clean [options] <in.mag>` (cmd.c:508-558): read the graph (filtering arcs, cutting one-read tips, amending and
 * merging on the way, unless told otherwise), clean it with -C, print it.  Host only. */
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>
#include "mag.h"

int fmdh_main_clean(int argc, char *argv[])
{
    fmdh_magopt_t opt;
    fmdh_mag_t *g;
    int c, rc;
    fmdh_mag_init_opt(&opt);
    while ((c = getopt(argc, argv, "ON:d:CFAl:e:i:o:R:n:w:r:S")) >= 0) {
        switch (c) {
        case 'F': opt.flag |= FMDH_MAG_F_NO_AMEND; break;
        case 'C': opt.flag |= FMDH_MAG_F_CLEAN; break;
        case 'A': opt.flag |= FMDH_MAG_F_AGGRESSIVE; break;
        case 'O': opt.flag |= FMDH_MAG_F_READ_ORI; break;
        case 'S': opt.flag |= FMDH_MAG_F_NO_SIMPL; break;
        case 'd': opt.min_dratio0 = (float)atof(optarg); break;
        case 'N': opt.max_arc = atoi(optarg); break;
        case 'l': opt.min_elen = atoi(optarg); break;
        case 'e': opt.min_ensr = atoi(optarg); break;
        case 'i': opt.min_insr = atoi(optarg); break;
        case 'o': opt.min_ovlp = atoi(optarg); break;
        case 'n': opt.n_iter = atoi(optarg); break;
        case 'R': opt.min_dratio1 = (float)atof(optarg); break;
        case 'w': opt.max_bcov = (float)atof(optarg); break;
        case 'r': opt.max_bfrac = (float)atof(optarg); break;
        }
    }
    if (argc == optind) {
        fprintf(stderr, "\n");
        fprintf(stderr, "Usage:   fermi-amd clean [options] <in.mog>\n\n");
        fprintf(stderr, "Options: -N INT      read maximum INT neighbors per node [%d]\n", opt.max_arc);
        fprintf(stderr, "         -d FLOAT    drop a neighbor if relative overlap ratio below FLOAT [%.2f]\n\n", opt.min_dratio0);
        fprintf(stderr, "         -C          clean the graph\n");
        fprintf(stderr, "         -l INT      minimum tip length [%d]\n", opt.min_elen);
        fprintf(stderr, "         -e INT      minimum tip read count [%d]\n", opt.min_ensr);
        fprintf(stderr, "         -i INT      minimum internal unitig read count [%d]\n", opt.min_insr);
        fprintf(stderr, "         -o INT      minimum overlap [%d]\n", opt.min_ovlp);
        fprintf(stderr, "         -R FLOAT    minimum relative overlap ratio [%.2f]\n", opt.min_dratio1);
        fprintf(stderr, "         -n INT      number of iterations [%d]\n", opt.n_iter);
        fprintf(stderr, "         -A          aggressive bubble popping\n");
        fprintf(stderr, "         -S          skip bubble simplification\n");
        fprintf(stderr, "         -w FLOAT    minimum coverage to keep a bubble [%.2f]\n", opt.max_bcov);
        fprintf(stderr, "         -r FLOAT    minimum fraction to keep a bubble [%.2f]\n", opt.max_bfrac);
        fprintf(stderr, "\n");
        return 1;
    }
    g = fmdh_mag_read(argv[optind], &opt);
    if (!g) return 1;
    fmdh_mag_clean(g, &opt);
    rc = g->err;
    if (rc) fprintf(stderr, "[E::%s] the graph is inconsistent (an arc to an end that no vertex has, or without its twin); nothing is written\n", __func__);
    else fmdh_mag_print(g, stdout);
    fmdh_mag_destroy(g);
    return rc ? 1 : 0;
}
