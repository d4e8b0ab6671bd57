/* clean_main.c -- `clean` alone, without the GPU library: what `make asan-mag` builds with -fsanitize=address,undefined to run the graph
 * module (host/mag.c, mag_bubble.c, swscore.c, clean_cmd.c and the reader they use) over the fixtures and over malformed input. */
#include "mag.h"
int main(int argc, char *argv[]) { return fmdh_main_clean(argc, argv); }
