// Round 4: the same conflict model as lds_layout_search.c over the wider SEPARABLE family off(y,x) = y*Q + A[x/R2] + B[x%R2] (tables instead of
// strides; still immediate offsets in the kernel), coordinate descent from the linear optimum and from random starts.  Result: nothing below
// the linear family's 5150 cycles (with y tables too: 5141).  A search over bank RESIDUES alone is misleading: it counts two different
// addresses with equal residues as a broadcast.  gcc -O2 -o lds_table_search lds_table_search.c; ./lds_table_search seed restarts 1 [rd_mask] [wr_mask]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
static int N=72,R1=8,R2=9,G=9,LPW=7,NW=11,Q=73;
static int A[8],B[9];
static inline int off(int y,int x){return y*Q+A[x/R2]+B[x%R2];}
static int group_cycles(const int*e,const int*act,int lo,int hi,int mod){
    int ns[32];int seen[32][64];memset(ns,0,sizeof ns);
    for(int l=lo;l<hi;++l){if(!act[l])continue;int b=((e[l]%mod)+mod)%mod,dup=0;for(int j=0;j<ns[b];++j)if(seen[b][j]==e[l])dup=1;if(!dup)seen[b][ns[b]++]=e[l];}
    int m=0;for(int b=0;b<mod;++b)if(ns[b]>m)m=ns[b];return m;
}
static int MAXF=7400;
// line roles whose elements k, k+1 go as ONE ds_read2_b64 / ds_write2_b64 (bit masks as in lds_layout_search.c, same costs: two accesses of
// four 16-lane groups, at least 8 / 13 cycles); default = the shipped build of P = 72: the stride-1 role only.  Arguments 4 and 5.
static int RD_MASK=1,WR_MASK=1;
static long cost(int tm,long*rd_,long*wr_){
    static unsigned char used[1<<15];int mx=0;
    int fx[72];for(int x=0;x<N;++x){fx[x]=A[x/R2]+B[x%R2];if(fx[x]>mx)mx=fx[x];}
    int fld=(N-1)*Q+mx+1;if(fld>MAXF)return 1L<<40;
    memset(used,0,fld);
    for(int y=0;y<N;++y)for(int x=0;x<N;++x){int a=y*Q+fx[x];if(used[a])return 1L<<40;used[a]=1;}
    long rd=0,wr=0;
    for(int w=0;w<NW;++w)for(int pat=0;pat<4;++pat){int R=(pat==0||pat==2)?R1:R2;
        int g16[16],g32[16];
        for(int k=0;k<R;++k){int e[64],act[64];
            for(int l=0;l<64;++l){int li=l/G,t=l%G,line=w*LPW+li;act[l]=(li<LPW)&&(line<N)&&((pat==0||pat==2)?(t<R2):(t<R1));if(!act[l]){e[l]=0;continue;}
                int idx=(pat==0||pat==2)?(k*R2+t):(t*R2+k);e[l]=(pat<2)?off(line,idx):off(idx,line);}
            g32[k]=group_cycles(e,act,0,32,32)+group_cycles(e,act,32,64,32);g16[k]=0;for(int g=0;g<4;++g)g16[k]+=group_cycles(e,act,16*g,16*g+16,16);}
        const int uses=(pat==1||pat==2)?2:1,rm=(RD_MASK>>pat)&1,wm=(WR_MASK>>pat)&1;
        for(int k=0;k<R;++k){const int pair=k+1<R;
            if(rm&&pair){int r_=g16[k]+g16[k+1];if(tm&&r_<8)r_=8;rd+=uses*r_;}
            else for(int j=k;j<=k+(rm?0:pair);++j){int r_=g32[j];if(tm&&r_<2)r_=2;rd+=uses*r_;}
            if(wm&&pair){int w_=g16[k]+g16[k+1];if(tm&&w_<13)w_=13;wr+=uses*w_;}
            else for(int j=k;j<=k+(wm?0:pair);++j){int w_=g16[j];if(tm&&w_<6)w_=6;wr+=uses*w_;}
            if(pair)++k;}}
    if(rd_)*rd_=rd;if(wr_)*wr_=wr;return rd+wr;
}
int main(int argc,char**argv){
    unsigned seed=argc>1?atoi(argv[1]):1;int iters=argc>2?atoi(argv[2]):20;int tm=argc>3?atoi(argv[3]):1;srand(seed);
    if(argc>4)RD_MASK=WR_MASK=atoi(argv[4]);if(argc>5)WR_MASK=atoi(argv[5]);
    long best=1L<<40;
    for(int rs=0;rs<iters;++rs){
        Q=73+rand()%12; if(rs==0)Q=73;
        // start: linear family member or random injective
        long cur;int tries=0;
        do{
            if(rs==0){for(int i=0;i<8;++i)A[i]=i;for(int j=0;j<9;++j)B[j]=65*j;}
            else{int pa=1+rand()%Q,pb=1+rand()%Q;for(int i=0;i<8;++i)A[i]=i*pa;for(int j=0;j<9;++j)B[j]=j*pb;}
            cur=cost(tm,0,0);
        }while(cur>=(1L<<40)&&++tries<100000);
        if(cur>=(1L<<40))continue;
        int improved=1;
        while(improved){improved=0;
            for(int v=0;v<17;++v){int*p=v<8?&A[v]:&B[v-8];int old=*p,bv=old;long bs=cur;
                for(int val=0;val<1200;++val){*p=val;long s=cost(tm,0,0);if(s<bs){bs=s;bv=val;}}
                *p=bv;if(bs<cur){cur=bs;improved=1;}}
        }
        if(cur<best){best=cur;long r,w;cost(tm,&r,&w);long r0,w0;long c0=cost(0,&r0,&w0);int mx=0;for(int x=0;x<N;++x){int f=A[x/R2]+B[x%R2];if(f>mx)mx=f;}
            printf("cost %ld (rd %ld wr %ld; pure %ld) Q=%d fld=%d A=",cur,r,w,c0,Q,(N-1)*Q+mx+1);for(int i=0;i<8;++i)printf("%d,",A[i]);printf(" B=");for(int j=0;j<9;++j)printf("%d,",B[j]);printf("\n");fflush(stdout);}
    }
    return 0;
}
